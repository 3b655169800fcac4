"""The routing table's inputs and the release library's list of k_raytrace_sm instantiations.  No test lives here.

table_rows() generates the launches of tests/golden/route_table.npz (profiles/route_move_record.py records what the routing ladder of the
commit before csrc/pt_host_route.cpp launched for each; tests/test_route_table.py holds mi3pt_host_route to it); RELEASE_BUILDS is the list
both tests/test_route_table.py and tests/test_gpu_build_table.py go by."""
import itertools

import numpy as np

from mi3pt_host import capi

REF_LEAF, REF_NONE = 0x80000000, 0xFFFFFFFF
SIX_WAVES_MIN_JOBS = 1500000            # csrc/pt_host_route.cpp: PT_SIX_WAVES_MIN_JOBS


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


BASE = dict(variant=13, tex_w=100, local_rows=52, nframes=5, num_cus=256, waves_per_cu=0, ntiles_active=0, six_waves=-1,
            walk_min=32, leaf_min=24, shade_split=64, tail_policy=7, job_chunk=4, tri_pair=1, wave_times=0, tile_cost=0, service=1, diag_lite=0,
            max_bounces=8, samples_per_frame=1, res_x_bits=f32_bits(100.0), res_y_bits=f32_bits(52.0),
            nnodes=2001, flags=7, root_ref=0, leaf_cap=13, cwide=1, cw8=1)
assert tuple(BASE) == capi.ROUTE_INPUTS

# what a scene has built: no nodes; a leaf root; binary packets only; + wide packets (routing does not ask for them: the same inputs);
# + compressed packets; + eight-wide packets
SCENE_CLASSES = (dict(nnodes=0, root_ref=REF_NONE, cwide=0, cw8=0), dict(nnodes=1, root_ref=REF_LEAF, cwide=0, cw8=0),
                 dict(cwide=0, cw8=0), dict(cwide=0, cw8=0), dict(cwide=1, cw8=0), dict(cwide=1, cw8=1))
# what takes a launch off the lean build, each singly, and none
LEAN_BREAKERS = (dict(), dict(wave_times=1), dict(wave_times=1, diag_lite=1), dict(tile_cost=1), dict(leaf_min=8), dict(shade_split=0),
                 dict(tail_policy=0), dict(job_chunk=1), dict(tri_pair=0), dict(service=0))
# the resolution limits of the lean culling builds, 2^-20 and 2^40, and the next float outside each
RES_BITS = (0x35800000, 0x357FFFFF, 0x53800000, 0x53800001)
TILES = ((8, 8), (100, 52), (1920, 1080), (3840, 2160), (3840, 270), (1920, 0))


def _rows(*axes):
    """the full product of the axes, each a list of dicts of inputs, over BASE (the last axis varies fastest)"""
    out = np.tile(np.array([BASE[k] for k in capi.ROUTE_INPUTS], np.int64), (int(np.prod([len(a) for a in axes])), 1))
    for axis, choice in zip(axes, np.indices([len(a) for a in axes]).reshape(len(axes), -1)):
        for j, inputs in enumerate(axis):
            for name, value in inputs.items():
                out[choice == j, capi.ROUTE_INPUTS.index(name)] = value
    return out


def _axis(name, values):
    return [{name: v} for v in values]


def table_rows():
    """(rows x len(capi.ROUTE_INPUTS)) int64: which kernel, the packing limits' edges, how many blocks"""
    which = _rows(_axis("variant", range(1, 15)), SCENE_CLASSES, _axis("flags", range(8)), _axis("leaf_cap", (0, 3, 4, 13)), LEAN_BREAKERS,
                  _axis("walk_min", (32, 44, 1)), _axis("six_waves", (-1, 0, 1)))
    edges = _rows(_axis("variant", (2, 4, 10, 13)), _axis("max_bounces", (8, 65535, 65536)), _axis("nframes", (1, 65535, 65536)),
                  _axis("samples_per_frame", (1, 1 << 24, (1 << 24) + 1)), _axis("res_x_bits", RES_BITS), _axis("res_y_bits", RES_BITS))
    walks = [dict(variant=v) for v in (2, 4, 10, 13, 14)] + [dict(variant=13, leaf_min=8)]      # five lean, one twin
    common = (_axis("num_cus", (0, 64, 256, 304)), _axis("waves_per_cu", (0, 4, 16, 20, 24, 25, 100)), _axis("six_waves", (-1, 0, 1)))
    blocks = []
    for w, h in TILES:
        tiles = ((w + 7) // 8) * ((h + 7) // 8)
        blocks.append(_rows(walks, [dict(tex_w=w, local_rows=h)], _axis("nframes", (1, 2, 3, 4, 32, 512)), _axis("ntiles_active", (0, 1, tiles // 2)),
                            _axis("walk_min", (32, 44)), *common))
    # jobs (frames x active tiles) exactly at and one below the six-wave threshold of either walk threshold
    for walk_min, jobs in ((32, SIX_WAVES_MIN_JOBS), (44, SIX_WAVES_MIN_JOBS // 10)):
        pairs = [dict(nframes=jobs // 3000, ntiles_active=3000), dict(nframes=1, ntiles_active=jobs - 1)]
        blocks.append(_rows(walks, [dict(tex_w=1920, local_rows=1080, walk_min=walk_min)], pairs, *common))
    return np.concatenate([which, edges] + blocks)


# The k_raytrace_sm instantiations of the release library (csrc/pt_kernels.h: PT_SM_BUILDS), as capi.ROUTE_BUILD:
#                       defer cull wide filt ymax diag toplds lite cw wmin waves w8
RELEASE_BUILDS = {"lean4": (0, 0, 0, 0, 0, 0, 0, 0, 0, 32, 5, 0), "lean7": (1, 0, 0, 0, 0, 0, 0, 0, 0, 32, 5, 0),
                  "lean9": (1, 1, 0, 0, 0, 0, 0, 0, 0, 32, 5, 0), "lean10": (1, 1, 1, 0, 0, 0, 0, 0, 0, 32, 5, 0),
                  "twin9": (1, 1, 0, 0, 0, 1, 0, 0, 0, 32, 5, 0), "twin10": (1, 1, 1, 0, 0, 1, 0, 0, 0, 32, 5, 0)}
for _variant, _ymax, _waves, _wmin in itertools.product((13, 14), (0, 1), (5, 6), (32, 44)):
    RELEASE_BUILDS[f"v{_variant}-ymax{_ymax}-waves{_waves}-wmin{_wmin}"] = (1, 1, 1, 1, _ymax, 0, 0, 0, 1, _wmin, _waves, int(_variant == 14))
assert len(RELEASE_BUILDS) == 22 and len(set(RELEASE_BUILDS.values())) == 22
