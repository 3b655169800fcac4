// A stand-alone driver of mi3pt_host_view_frame (csrc/pt_host_reproject.cpp) for AddressSanitizer + UndefinedBehaviorSanitizer: every
// kind of input the function accepts or refuses, from buffers of exactly the size it is told.  tests/tools/sanitize_view_frame.sh builds
// and runs it; it prints one "ok" line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "mi3pt.h"

int pt_set_error(int code, const std::string &msg) { std::fprintf(stderr, "(expected) error %d: %s\n", code, msg.c_str()); return code; }

static std::vector<unsigned char> block(float aspect, const float pos[3], const float dir[3], float fov, size_t nbytes = MI3PT_RAYTRACE_UNIFORMS_SIZE)
{
    std::vector<unsigned char> u(MI3PT_RAYTRACE_UNIFORMS_SIZE, 0);
    std::memcpy(u.data() + 8, &aspect, 4);
    std::memcpy(u.data() + 32, pos, 12);
    std::memcpy(u.data() + 48, dir, 12);
    std::memcpy(u.data() + 60, &fov, 4);
    u.resize(nbytes);          // (a heap buffer of exactly that size: a read past it is caught)
    return u;
}

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float pos[3] = { 0.0f, 1.0f, 4.0f };
    const float dirs[][3] = { { 0.0f, -0.2425356f, -0.9701425f }, { 0.0f, -1.0f, 0.0f }, { 0.0f, 3.0f, 0.0f }, { 1e-30f, 1e-30f, -1e-30f },
                              { 1e30f, -1e30f, 1e30f }, { 0.004f, -1.0f, 0.001f } };
    int failures = 0;
    for (const auto &dir : dirs)
        for (float fov : { 1.0f, 45.0f, 179.0f, 1e-30f }) {
            std::vector<unsigned char> u = block(1.5f, pos, dir, fov);
            std::vector<float> out(16, nan);
            if (mi3pt_host_view_frame(u.data(), u.size(), out.data()) != MI3PT_OK) failures++;
            for (float v : out)
                if (!std::isfinite(v)) failures++;
        }
    std::vector<float> out(16);
    const float zero[3] = { 0.0f, 0.0f, 0.0f }, bad_dir[3] = { nan, 0.0f, 1.0f }, inf_dir[3] = { inf, 0.0f, 1.0f }, bad_pos[3] = { 0.0f, inf, 0.0f };
    const float *good = dirs[0];
    if (mi3pt_host_view_frame(block(1.5f, pos, zero, 45.0f).data(), 96, out.data()) != MI3PT_ERR_INVALID) failures++;
    if (mi3pt_host_view_frame(block(1.5f, pos, bad_dir, 45.0f).data(), 96, out.data()) != MI3PT_ERR_INVALID) failures++;
    if (mi3pt_host_view_frame(block(1.5f, pos, inf_dir, 45.0f).data(), 96, out.data()) != MI3PT_ERR_INVALID) failures++;
    if (mi3pt_host_view_frame(block(1.5f, bad_pos, good, 45.0f).data(), 96, out.data()) != MI3PT_ERR_INVALID) failures++;
    for (float fov : { 0.0f, 180.0f, -1.0f, nan, inf })
        if (mi3pt_host_view_frame(block(1.5f, pos, good, fov).data(), 96, out.data()) != MI3PT_ERR_INVALID) failures++;
    for (size_t n : { (size_t)0, (size_t)1, (size_t)95, (size_t)97 }) {        // a wrong size is refused before a byte is read
        std::vector<unsigned char> u = block(1.5f, pos, good, 45.0f, n);
        if (mi3pt_host_view_frame(u.data(), n, out.data()) != MI3PT_ERR_INVALID) failures++;
    }
    if (mi3pt_host_view_frame(nullptr, 96, out.data()) != MI3PT_ERR_INVALID) failures++;
    if (mi3pt_host_view_frame(block(1.5f, pos, good, 45.0f).data(), 96, nullptr) != MI3PT_ERR_INVALID) failures++;
    if (failures) { std::printf("mi3pt_host_view_frame under ASan + UBSan: %d FAILURES\n", failures); return 1; }
    std::printf("mi3pt_host_view_frame under ASan + UBSan: ok\n");
    return 0;
}
