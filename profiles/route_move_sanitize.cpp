// The router (csrc/pt_host_route.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own: every row of the
// routing table (tests/route_table.py: table_rows(), written out as raw int64) through mi3pt_host_route.
//   python3 -c "import sys; sys.path[:0] = ['webgpu-pathtracer_amd/py', 'tests']; import route_table; route_table.table_rows().tofile('/tmp/route_rows.i64')"
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -w -Iinclude -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
//       profiles/route_move_sanitize.cpp webgpu-pathtracer_amd/csrc/pt_host_route.cpp -o /tmp/route_sanitize && /tmp/route_sanitize /tmp/route_rows.i64
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../include/mi3pt.h"

int pt_set_error(int code, const std::string &msg) { fprintf(stderr, "error %d: %s\n", code, msg.c_str()); return code; }

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) { fprintf(stderr, "usage: %s rows.i64\n", argv[0]); return 2; }
    std::vector<int64_t> in;
    int64_t buf[MI3PT_HOST_ROUTE_INPUTS];
    while (fread(buf, sizeof buf, 1, f) == 1) in.insert(in.end(), buf, buf + MI3PT_HOST_ROUTE_INPUTS);
    fclose(f);
    const size_t rows = in.size() / MI3PT_HOST_ROUTE_INPUTS;
    std::vector<int64_t> out(rows * MI3PT_HOST_ROUTE_OUTPUTS);
    if (mi3pt_host_route(in.data(), rows, out.data()) != MI3PT_OK) return 1;
    size_t sm = 0, kernels = 0;
    for (size_t k = 0; k < rows; k++) { sm += out[k * MI3PT_HOST_ROUTE_OUTPUTS] == 1; kernels += out[k * MI3PT_HOST_ROUTE_OUTPUTS + 19] == 1; }
    printf("%zu rows routed, %zu to the state-machine kernel, %zu with a kernel\n", rows, sm, kernels);
    return kernels == rows ? 0 : 1;
}
