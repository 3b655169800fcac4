#!/usr/bin/env python3
"""Records what the routing ladder of the commit BEFORE csrc/pt_host_route.cpp launched, as tests/golden/route_table.npz.

    python3 profiles/route_move_record.py [--commit 946743d] [--experiments] [--out tests/golden/route_table.npz | --compare]

The parent's own functions run, on the CPU: its csrc/ is checked out into a scratch directory, pt_kernels.hip gets a recording entry point
appended and hipLaunchKernelGGL redefined (in front of namespace pt) to note its stringified first argument and the grid instead of
launching, and the file alone is compiled into a library of its own (nothing in it is ever launched: no device is needed).  Per row of
tests/route_table.py's table_rows() the entry point fills an RtLaunch as mi3pt_host_route does, calls the parent's raytrace_route, launch_raytrace_setup and launch_raytrace, and returns the seven reported
fields, the first kernel launched with its grid, the number of launches and whether the setup kernel ran.  The template argument list of
k_raytrace_sm<...> is the instantiation the parent picks (omitted arguments: the template's defaults).

--compare: instead of writing the table, hold the working tree's library (MI3PT_LIBRARY or the built one) to the recording and print
every row that differs -- how the -DMI3PT_EXPERIMENTS library was compared by hand (profiles/route_move.log)."""
import argparse
import collections
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "webgpu-pathtracer_amd", "py"), os.path.join(ROOT, "tests")]
from mi3pt_host import capi  # noqa: E402
import route_table  # noqa: E402

RECORDER = r"""
#include <string>
static std::string pt_rec_name; static unsigned pt_rec_grid; static int pt_rec_launches, pt_rec_setup;
static void pt_rec(const char *k, dim3 g)
{
    if (std::string(k) == "k_rt_service_setup") { pt_rec_setup++; return; }
    if (!pt_rec_launches++) { pt_rec_name = k; pt_rec_grid = g.x; }
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, ...) pt_rec(#k, g)
"""
ENTRY = r"""
#include <cstring>
extern "C" void mi3pt_record_constants(int64_t *out)
{
    const int64_t c[5] = { PT_DEFAULT_WALK_MIN, PT_DEEP_WALK_MIN, pt::SM_TUNED_WAVES_PER_SIMD, pt::SM_SIX_WAVES_PER_SIMD, PT_TOP_CW };
    std::memcpy(out, c, sizeof c);
}
extern "C" void mi3pt_record_route(const int64_t *in, size_t rows, int64_t *out, char *names, size_t name_bytes)
{
    static char bound;
    for (size_t k = 0; k < rows; k++, in += 28, out += 10, names += name_bytes) {
        pt::RtLaunch L;
        std::memset(&L, 0, sizeof L);
        auto present = [&](int i) { return in[i] ? static_cast<void *>(&bound) : nullptr; };
        auto f32 = [&](int i) { const uint32_t u = (uint32_t)in[i]; float f; std::memcpy(&f, &u, 4); return f; };
        L.tile.tex_w = (int32_t)in[1]; L.tile.local_rows = (int32_t)in[2];
        L.nframes = (int32_t)in[3]; L.num_cus = (int32_t)in[4]; L.waves_per_cu = (int32_t)in[5]; L.ntiles_active = (int32_t)in[6]; L.six_waves = (int32_t)in[7];
        L.walk_min = (int32_t)in[8]; L.leaf_min = (int32_t)in[9]; L.shade_split = (int32_t)in[10]; L.tail_policy = (int32_t)in[11];
        L.job_chunk = (int32_t)in[12]; L.tri_pair = (int32_t)in[13];
        L.wave_times = static_cast<uint64_t *>(present(14)); L.tile_cost = static_cast<uint32_t *>(present(15));
        L.service = static_cast<pt::RtService *>(present(16)); L.diag_lite = (int32_t)in[17];
        L.un.max_bounces = (int32_t)in[18]; L.un.samples_per_frame = (int32_t)in[19];
        L.un.res_x = f32(20); L.un.res_y = f32(21);
        L.scene.nnodes = (uint32_t)in[22]; L.scene.flags = (uint32_t)in[23]; L.scene.root_ref = (uint32_t)in[24]; L.scene.leaf_cap = (int32_t)in[25];
        L.scene.cwide = L.scene.tripk64 = static_cast<const float4 *>(present(26));
        L.scene.cw8 = L.scene.tripk8 = static_cast<const float4 *>(present(27));
        pt_rec_name.clear(); pt_rec_grid = 0; pt_rec_launches = pt_rec_setup = 0;
        const pt::RtRoute r = pt::raytrace_route(L, (int)in[0]);
        pt::launch_raytrace_setup(L, false, (int)in[0], nullptr);
        pt::launch_raytrace(L, false, (int)in[0], nullptr);
        const int64_t o[10] = { r.kind, r.variant, r.lean, r.blocks, r.waves, r.ymax, r.walk_min, pt_rec_grid, pt_rec_launches, pt_rec_setup };
        std::memcpy(out, o, sizeof o);
        std::strncpy(names, pt_rec_name.c_str(), name_bytes - 1);
    }
}
"""
NAME_BYTES = 192


def build_recorder(commit, experiments, tmp):
    subprocess.run(f"git -C {ROOT} archive {commit} webgpu-pathtracer_amd/csrc include | tar -x -C {tmp}", shell=True, check=True)
    csrc = os.path.join(tmp, "webgpu-pathtracer_amd", "csrc")
    text = open(os.path.join(csrc, "pt_kernels.hip")).read()
    head, sep, tail = text.partition("\nnamespace pt {\n")
    assert sep, "pt_kernels.hip: namespace pt not found"
    open(os.path.join(csrc, "pt_kernels_record.hip"), "w").write(head + RECORDER + sep + tail + ENTRY)
    flags = [l for l in open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ").splitlines() if l.startswith("CXXFLAGS")][0].split("?=")[1].split()
    lib = os.path.join(tmp, "librecord.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *flags, "-Wno-unused-variable", "-shared", "-o", lib, "pt_kernels_record.hip"]
                   + (["-DMI3PT_EXPERIMENTS"] if experiments else []), cwd=csrc, check=True)
    return ctypes.CDLL(lib)


def record(lib, rows):
    """the parent's answers: reported (n x 7), build (n x 12; zeros where no k_raytrace_sm ran), grid, launches, setup"""
    consts = np.zeros(5, np.int64)
    lib.mi3pt_record_constants(ctypes.c_void_p(consts.ctypes.data))
    words = {"true": 1, "false": 0, "PT_DEFAULT_WALK_MIN": consts[0], "PT_DEEP_WALK_MIN": consts[1], "SM_TUNED_WAVES_PER_SIMD": consts[2],
             "SM_SIX_WAVES_PER_SIMD": consts[3], "PT_TOP_CW": consts[4]}      # (macros arrive expanded, constants by name)
    defaults = [None] * 6 + [0, 0, 0, consts[0], consts[2], 0]       # TOPLDS, LITE, CW, WMIN, WAVES, W8 of the template
    out = np.zeros((len(rows), 10), np.int64)
    names = np.zeros((len(rows), NAME_BYTES), np.uint8)
    lib.mi3pt_record_route(ctypes.c_void_p(rows.ctypes.data), ctypes.c_size_t(len(rows)), ctypes.c_void_p(out.ctypes.data),
                           ctypes.c_void_p(names.ctypes.data), ctypes.c_size_t(NAME_BYTES))
    parsed = {}
    build = np.zeros((len(rows), 12), np.int64)
    kernels = collections.Counter()
    for k, raw in enumerate(names):
        name = raw.tobytes().split(b"\0")[0].decode()
        if name not in parsed:
            args = []
            if "k_raytrace_sm<" in name:
                args = [int(words.get(w.strip(), w)) for w in name[name.index("<") + 1:name.rindex(">")].split(",")]
                args += defaults[len(args):]
            parsed[name] = args or [0] * 12
        build[k] = parsed[name]
        kernels[name] += 1
    return out[:, :7], build, out[:, 7], out[:, 8], out[:, 9], kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="946743d")
    ap.add_argument("--experiments", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "route_table.npz"))
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    rows = route_table.table_rows()
    with tempfile.TemporaryDirectory() as tmp:
        reported, build, grid, launches, setup, kernels = record(build_recorder(a.commit, a.experiments, tmp), rows)
    print(f"{len(rows)} rows, {len(kernels)} distinct first kernels, {len(np.unique(build[reported[:, 0] == 1], axis=0))} k_raytrace_sm instantiations")
    for name, n in sorted(kernels.items()):
        print(f"  {n:7d}  {name or '(nothing launched)'}")
    if not a.compare:
        # (field-major: a column of a product table is long runs of one value, which is what makes the file small)
        np.savez_compressed(a.out, inputs=rows.T.copy(), reported=reported.T.astype(np.int32), build=build.T.astype(np.int8),
                            grid=grid.astype(np.int32), launches=launches.astype(np.int32), setup=setup.astype(np.int8))
        print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")
        return
    new = capi.host_route(rows)
    launched = launches > 0
    want = np.concatenate([reported, np.where(launched[:, None], build, new[:, 7:19])], axis=1)      # (nothing launched: no instantiation to compare)
    differs = np.flatnonzero((new[:, :19] != want).any(axis=1))
    print(f"{capi.LIB_PATH}: {len(differs)} of {len(rows)} rows differ in a reported field or the build")
    groups = collections.Counter()
    for k in differs:
        fields = tuple(capi.ROUTE_OUTPUTS[j] for j in np.flatnonzero(new[k, :19] != want[k]))
        groups[(int(rows[k, 0]), int(rows[k, 23]) & 4, int(rows[k, 8]), int(rows[k, 17]), fields,
                tuple(int(x) for x in want[k][list(map(capi.ROUTE_OUTPUTS.index, fields))]), tuple(int(x) for x in new[k][list(map(capi.ROUTE_OUTPUTS.index, fields))]))] += 1
    for (variant, flag, walk_min, lite, fields, was, now), n in sorted(groups.items()):
        print(f"  {n:6d} rows  requested {variant:2d}  flags & 4 = {flag}  walk_min {walk_min:2d}  diag_lite {lite}:  {', '.join(fields)}  {was} -> {now}")
    sm = new[:, 0] == 1
    print("grid of the first launch != blocks, where something was launched:", int((launched & (grid != new[:, 3])).sum()),
          "| setup differs:", int((setup != new[:, 20]).sum()), "| kind-1 rows without a kernel:", int((sm & (new[:, 19] != 1)).sum()))


if __name__ == "__main__":
    main()
