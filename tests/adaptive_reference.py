"""Reference for adaptive sampling (mi3pt_set_sample_mask, mi3pt_host_freeze_tiles, renderUntil(adaptive=True)), written from the header
comment of include/mi3pt.h: the rule that freezes converged tiles, the composition of a launch's tile lists, what a masked run leaves in
the image, and the hosts' adaptive loop over a sequence of tile maps.

numpy, on top of convergence_reference's verdict.  Nothing here looks at the device.  No test lives in this file.
"""
import numpy as np

import convergence_reference as cr


def freeze_tiles(records, threshold, min_frames, guard, mask=None):
    """(new mask (tiles_y, tiles_x) uint8, sampled tiles): the rule on a (tiles_y, tiles_x, 4) tile map and the mask so far (None: all
    sampled).  under(t) = count > 0 and not above; a tile with count == 0 is frozen at once; a sampled tile with count > 0 is frozen iff
    under(t) and, for guard 1, every neighbour inside the map is under or has count == 0; a frozen tile stays frozen."""
    if guard not in (0, 1):
        raise ValueError("guard must be 0 or 1")
    rec = np.asarray(records, np.float32)
    ty, tx = rec.shape[:2]
    old = np.ones((ty, tx), bool) if mask is None else np.asarray(mask).reshape(ty, tx) != 0
    counted, _, above, _ = cr.verdict(rec, threshold, min_frames)
    under = counted & ~above
    new = np.zeros((ty, tx), np.uint8)
    for y in range(ty):
        for x in range(tx):
            if not old[y, x] or not counted[y, x]:
                continue                                     # stays frozen / has nothing to sample
            freeze = bool(under[y, x])
            if freeze and guard == 1:
                for uy in range(max(y - 1, 0), min(y + 2, ty)):
                    for ux in range(max(x - 1, 0), min(x + 2, tx)):
                        if (uy, ux) != (y, x) and counted[uy, ux] and not under[uy, ux]:
                            freeze = False
            new[y, x] = 0 if freeze else 1
    return new, int(new.sum())


def compose_lists(mask, empty):
    """(A, S): the sampled tiles that are not empty and the sampled tiles that are, each ascending -- a launch's device list is A then S.
    mask / empty: flat or 2-d, None = every tile sampled / no tile empty (then the other argument gives the size)."""
    n = np.asarray(mask if mask is not None else empty).size
    m = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    e = np.zeros(n, bool) if empty is None else np.asarray(empty).reshape(-1) != 0
    return np.flatnonzero(m & ~e).astype(np.uint32), np.flatnonzero(m & e).astype(np.uint32)


def tile_texels(mask, rows, width):
    """(rows, width) bool: the texels of the tiles a (tiles_y, tiles_x) mask marks"""
    m = np.asarray(mask) != 0
    return np.kron(m, np.ones((8, 8), bool))[:rows, :width]


def composite(snapshots, last):
    """What a run that only ever freezes leaves: per texel, the unmasked run's texel after the last chunk its tile was sampled in.
    snapshots[k]: the unmasked image after chunk k (k = 0: before the first); last: (tiles_y, tiles_x) int, that chunk per tile."""
    rows, width = snapshots[0].shape[:2]
    out = np.array(snapshots[0], copy=True)
    last = np.asarray(last)
    for k in range(1, len(snapshots)):
        sel = tile_texels(last == k, rows, width)
        out[sel] = snapshots[k][sel]
    return out


def render_until_adaptive(tile_map_at, shape, threshold, min_frames, max_frames, check_every, lookahead=True, guard=1):
    """Renderer.renderUntil(adaptive=True) over a replay.  tile_map_at(frames) -> the UNMASKED run's tile map after `frames` frames: a
    tile's record depends on its own texels only, so the masked run's record of a tile is the unmasked one's at the frame count the tile
    was last sampled at.  shape = (tiles_y, tiles_x).  Returns a dict: converged, frames, sampled (tile-frames), history (the mask after
    each freeze), last (frames each tile was sampled for), tiles (the final image's tile map)."""
    mask = np.ones(shape, np.uint8)
    last = np.zeros(shape, np.int64)
    cache = {}

    def image():
        out = np.zeros(shape + (4,), np.float32)
        for n in np.unique(last):
            if n not in cache:
                cache[n] = np.asarray(tile_map_at(int(n)), np.float32)
            out[last == n] = cache[n][last == n]
        return out

    frames = sampled = 0
    pending = None
    history = []
    done = False
    while frames < max_frames and not done:
        n = min(check_every, max_frames - frames)
        frames += n
        last[mask != 0] = frames
        sampled += n * int(mask.sum())
        if lookahead:
            if pending is not None:
                mask, left = freeze_tiles(pending, threshold, min_frames, guard, mask)
                pending = None
                history.append(mask.copy())
                done = left == 0
            if not done:
                pending = image()
        else:
            mask, left = freeze_tiles(image(), threshold, min_frames, guard, mask)
            history.append(mask.copy())
            done = left == 0
    return {"converged": done, "frames": frames, "sampled": sampled, "history": history, "last": last, "tiles": image()}
