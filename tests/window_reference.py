"""TEST INFRASTRUCTURE: a plain CPU restatement of what one launch of the window kernel computes for one rank of a ray-sharded
mapping iteration (nsr_get_samples_window_sharded): the pixel draw, the sampled rays with the bounding-box pre-filter, and the
kept rays' maximum depth over the union of every rank's draw.  numpy / torch on the CPU and the oracle's ``pixel_rays``;
nothing of the library under test.  The maximum is a selection, not arithmetic: every comparison against this module is
bit for bit."""
from collections import namedtuple

import numpy as np
import torch

from oracle import nice_oracle as orc

M64 = (1 << 64) - 1


def _philox_word(c, key):
    """philox4x32-10, first output word, restated from Salmon et al. (SC'11) -- the tests' own copy, vectorised over counters
    c [n, 4] uint32; key (k0, k1)."""
    c = c.astype(np.uint64).copy()
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    M0, M1, m32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[:, 0], M1 * c[:, 2]
        n0 = ((p1 >> np.uint64(32)) ^ c[:, 1] ^ k0) & m32
        n2 = ((p0 >> np.uint64(32)) ^ c[:, 3] ^ k1) & m32
        c = np.stack([n0, p1 & m32, n2, p0 & m32], 1)
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c[:, 0]


def draw(seed, call, K, n, crop_pixels):
    """The pixels a rank with state ``[seed, call, ...]`` draws for a window of K frames with n pixels each: int64 [K*n], ray
    t = k*n + i gets philox(counter = (t low, t high, call low, call high), key = (seed low, seed high)) mapped to
    [0, crop_pixels) by (r * crop_pixels) >> 32."""
    seed, call = int(seed) & M64, int(call) & M64
    t = np.arange(K * n, dtype=np.uint64)
    ctr = np.zeros((K * n, 4), np.uint32)
    ctr[:, 0], ctr[:, 1] = t & np.uint64(0xFFFFFFFF), t >> np.uint64(32)
    ctr[:, 2], ctr[:, 3] = call & 0xFFFFFFFF, call >> 32
    r = _philox_word(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return ((r * np.uint64(crop_pixels)) >> np.uint64(32)).astype(np.int64)


def exit_distance(rays_o, rays_d, bound):
    """fp64 distance at which each ray leaves ``bound`` [3, 2]: the slab test of Mapper.py:471-481"""
    t = (bound.unsqueeze(0) - rays_o.unsqueeze(-1)) / rays_d.unsqueeze(-1)
    t, _ = torch.min(torch.max(t, dim=2)[0], dim=1)
    return t


def window(indices, K, n, crop, intr, frames, bound):
    """The rays of the crop pixels ``indices`` [K*n] (frame-major) of ``frames`` [(c2w, depth [H,W], color [H,W,3])] with the
    bounding-box pre-filter -> rays_o, rays_d, gt_depth, gt_color, keep (bool), kept_max (fp32 scalar: the maximum depth over
    the rays with keep and depth > 0, 0.0 without one).  crop = (H0, H1, W0, W1), intr = (fx, fy, cx, cy)."""
    H0, H1, W0, W1 = crop
    fx, fy, cx, cy = intr
    indices = torch.as_tensor(np.asarray(indices), dtype=torch.int64)
    parts = [orc.pixel_rays(indices[k * n:(k + 1) * n], H0, H1, W0, W1, fx, fy, cx, cy, frames[k][0].detach(), frames[k][1], frames[k][2])
             for k in range(K)]
    o, d, gd, gc = (torch.cat([p[i] for p in parts]) for i in range(4))
    keep = exit_distance(o, d, torch.as_tensor(bound, dtype=torch.float64)) >= gd
    cnt = keep & (gd > 0)
    kept_max = gd[cnt].max().numpy() if bool(cnt.any()) else np.float32(0.0)
    return o.contiguous(), d.contiguous(), gd, gc, keep, np.float32(kept_max)


UnionMax = namedtuple("UnionMax", "value seed frame i per_seed")


def union_max(seeds, call, K, n, crop, intr, frames, bound):
    """The batch-global depth cap of a sharded iteration: the maximum of ``window(draw(seed, call))``'s counted depths over all
    ``seeds`` (fp32; 0.0 without a counted ray), the position in ``seeds`` / frame / in-frame index i of the first ray that attains
    it (None each without one), and every seed's own maximum."""
    H0, H1, W0, W1 = crop
    best, who, per = np.float32(0.0), (None, None, None), []
    for s, seed in enumerate(seeds):
        _, _, gd, _, keep, kmax = window(draw(seed, call, K, n, (H1 - H0) * (W1 - W0)), K, n, crop, intr, frames, bound)
        per.append(kmax)
        if kmax > best:
            t = int(torch.nonzero(keep & (gd == float(kmax)))[0])
            best, who = kmax, (s, t // n, t % n)
    return UnionMax(best, *who, per)


def exclusive_rays(seeds, call, K, n, crop, intr, frames, bound, holder, min_i=0):
    """Rays (frame k, in-frame index i >= min_i) of ``seeds[holder]``'s draw whose pixel no other ray of ANY seed hits in frame k:
    [(k, i, crop index, fp64 exit distance)], longest exit distance first."""
    H0, H1, W0, W1 = crop
    P = (H1 - H0) * (W1 - W0)
    draws = [draw(s, call, K, n, P).reshape(K, n) for s in seeds]
    hits = np.zeros((K, P), np.int64)
    for dr in draws:
        for k in range(K):
            hits[k] += np.bincount(dr[k], minlength=P)
    own = draws[holder]
    o, d, _, _, _, _ = window(own.reshape(-1), K, n, crop, intr, frames, bound)
    t = exit_distance(o, d, torch.as_tensor(bound, dtype=torch.float64)).numpy().reshape(K, n)
    out = [(k, i, int(own[k, i]), float(t[k, i])) for k in range(K) for i in range(min_i, n) if hits[k, own[k, i]] == 1]
    return sorted(out, key=lambda e: -e[3])


def set_depth(frames, k, crop, index, value):
    """``frames`` with the depth of crop pixel ``index`` of frame k set to ``value`` (the other frames' tensors are shared)"""
    H0, H1, W0, W1 = crop
    row, col = index // (W1 - W0) + H0, index % (W1 - W0) + W0
    depth = frames[k][1].clone()
    depth[row, col] = value
    out = list(frames)
    out[k] = (frames[k][0], depth, frames[k][2])
    return out


def plant_maximum(seeds, call, K, n, crop, intr, frames, bound, holder, min_i=0, required=True):
    """Frames in which a ray of ``seeds[holder]`` with in-frame index >= min_i holds the union maximum alone -- as they are if the
    draw gives that by itself, else with ONE depth pixel raised: a pixel only that ray hits, whose ray leaves the bound beyond
    the current union maximum, gets a depth between the two (so it is kept, and larger than every other counted depth).
    Without such a pixel: an error, or with ``required=False`` the frames as they are."""
    u = union_max(seeds, call, K, n, crop, intr, frames, bound)
    others = max([np.float32(0.0)] + [m for s, m in enumerate(u.per_seed) if s != holder])
    if u.seed == holder and u.i >= min_i and u.value > others:
        return frames
    for k, i, index, t in exclusive_rays(seeds, call, K, n, crop, intr, frames, bound, holder, min_i):
        v = np.float32(0.5 * (float(u.value) + t))
        if float(u.value) < float(v) < t:
            frames = set_depth(frames, k, crop, index, float(v))
            chk = union_max(seeds, call, K, n, crop, intr, frames, bound)
            assert (chk.value, chk.seed, chk.frame, chk.i) == (v, holder, k, i), (chk, v, holder, k, i)
            return frames
        break                                                   # sorted by exit distance: no later candidate reaches further
    if not required:
        return frames
    raise AssertionError("no pixel exclusive to seed %d leaves the bound beyond the union maximum %r" % (holder, u.value))


def expected_launch(own_seed, peer_seeds, call, K, n, crop, intr, frames, bound):
    """What one sharded launch of the rank with ``own_seed`` must leave: its own indices, rays and mask, and the header's maximum"""
    H0, H1, W0, W1 = crop
    ind = draw(own_seed, call, K, n, (H1 - H0) * (W1 - W0))
    o, d, gd, gc, keep, own_max = window(ind, K, n, crop, intr, frames, bound)
    u = union_max([own_seed] + list(peer_seeds), call, K, n, crop, intr, frames, bound)
    return {"indices": ind, "rays_o": o.numpy(), "rays_d": d.numpy(), "gt_depth": gd.numpy(), "gt_color": gc.numpy(),
            "keep": keep.numpy().astype(np.uint8), "own_max": own_max, "union": u}


GUARD = 8                       # elements behind every output that no launch may touch
PREFILL = {"indices": -1, "rays_o": np.nan, "rays_d": np.nan, "gt_depth": np.nan, "gt_color": np.nan, "keep": 9}
WIDTH = {"indices": 1, "rays_o": 3, "rays_d": 3, "gt_depth": 1, "gt_color": 3, "keep": 1}
SPAN_GUARD = 7.0


def same(a, b):
    """bit-equal arrays of one dtype (NaN patterns included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def untouched(got):
    """every output of a refused launch still holds its pre-fill"""
    for name, fill in PREFILL.items():
        a = np.asarray(got[name])
        if not (np.all(np.isnan(a)) if isinstance(fill, float) else np.all(a == fill)):
            return False
    return bool(np.all(np.isnan(got["Z"][:-GUARD])) and np.all(got["Z"][-GUARD:] == SPAN_GUARD))


def check_launch(got, exp, N, zero_n, seed, call_after):
    """``got``: the flat host copies of a launch's buffers, each pre-filled (PREFILL) and GUARD elements longer than its output;
    "Z": header [4] | span [zero_n] | GUARD x 7.0 over a NaN pre-fill; "state": the four state words after the launch."""
    for name, fill in PREFILL.items():
        a, w = np.asarray(got[name]), WIDTH[name]
        assert a.size == N * w + GUARD, name
        assert same(a[:N * w], exp[name].reshape(-1)), name
        tail = a[N * w:]
        assert np.all(np.isnan(tail)) if isinstance(fill, float) else np.all(tail == fill), "guard behind " + name
    Z = np.asarray(got["Z"])
    assert Z.size == 4 + zero_n + GUARD
    assert same(Z[:4], np.array([0.0, 0.0, exp["union"].value, 0.0], np.float32)), (Z[:4], exp["union"])
    assert same(Z[4:4 + zero_n], np.zeros(zero_n, np.float32)), "zero span"
    assert np.all(Z[4 + zero_n:] == SPAN_GUARD), "guard behind the zero span"
    assert [int(v) & M64 for v in got["state"]] == [int(seed) & M64, int(call_after) & M64, 0, 0], got["state"]


# the launch geometries of the sweep: (n_peers, n, K) -- one and several sampling blocks per rank (256 threads), a partial last
# block, n = 257 (one thread of the second block), the maximum peer count, K = 1 (the hand-off count draw_bx * K without rows)
GEOMETRIES = [(1, 1, 1), (1, 300, 3), (2, 256, 3), (3, 257, 2), (7, 25, 5), (7, 700, 3), (15, 40, 3), (15, 300, 1)]
ZERO_SPANS = (0, 5, 70001)


def geometry_case(frames, crop, intr, bound, n_peers, n, K, call=5):
    """seeds (own first), frames and the reference of one geometry of the sweep.  A peer holds the union maximum wherever the
    geometry has a ray to plant it on (asserted for all but the tiniest) -- the FIRST peer in every other geometry of GEOMETRIES,
    the LAST in the rest; in its second x-block if one of a few seed sets allows that."""
    base, fr0 = 100000 * n_peers + 100 * n + K, frames_with(frames, K)
    holder = 1 if GEOMETRIES.index((n_peers, n, K)) % 2 == 0 else n_peers
    for attempt, min_i in [(a, 256) for a in range(8 if n > 256 else 0)] + [(0, 0)]:
        seeds = seeds_for(8 * base + attempt, 1 + n_peers)
        fr = plant_maximum(seeds, call, K, n, crop, intr, fr0, bound, holder, min_i, required=False)
        u = union_max(seeds, call, K, n, crop, intr, fr, bound)
        if u.seed == holder and u.i >= min_i and u.value > max(m for q, m in enumerate(u.per_seed) if q != holder):
            break
    exp = expected_launch(seeds[0], seeds[1:], call, K, n, crop, intr, fr, bound)
    if n * K >= 40:
        assert exp["union"].seed == holder and exp["union"].value > exp["own_max"], (n_peers, n, K)
    return seeds, fr, exp


def seeds_for(tag, count):
    """distinct 63-bit seeds with both halves populated, fixed per tag"""
    g = np.random.default_rng(tag)
    out = [int(v) for v in g.integers(1 << 40, (1 << 63) - 1, size=count, dtype=np.int64)]
    assert len(set(out)) == count
    return out


def frames_with(frames, K):
    """K frames out of a shorter list: the list repeated, depths scaled a little per repeat so that no two frames are equal"""
    out = []
    for k in range(K):
        c2w, d, col = frames[k % len(frames)]
        out.append((c2w, d * (1.0 + 0.013 * (k // len(frames))), col))
    return out


# every rank of one world: (world, n, K, rank that holds the union maximum, least in-frame index of the holding ray)
WORLDS = [(2, 300, 3, 1, 256), (3, 300, 2, 0, 256), (3, 40, 3, 2, 0), (8, 25, 5, 7, 0), (8, 300, 3, 0, 256), (16, 40, 3, 0, 0), (16, 25, 3, 15, 0)]
WORLD_CALL = 11


def world_cases(frames, crop, intr, bound):
    """[(world, n, K, seeds, frames, {rank: expected_launch})] over WORLDS, with the maximum planted where the draw does not give
    it, and -- on the reference alone, before any kernel runs -- the situations that make the comparison discriminating: over
    the launches of all cases the union maximum is strictly greater than the calling rank's own maximum while held by the
    caller's FIRST peer, by its LAST peer, and by a peer ray of the second x-block (i >= 256)."""
    cases, seen = [], {"first": 0, "last": 0, "second_block": 0, "greater": 0}
    for w, n, K, holder, min_i in WORLDS:
        seeds = seeds_for(1000 * w + n, w)
        fr = plant_maximum(seeds, WORLD_CALL, K, n, crop, intr, frames_with(frames, K), bound, holder, min_i)
        exp = {}
        for r in range(w):
            peers = [s for q, s in enumerate(seeds) if q != r]
            e = exp[r] = expected_launch(seeds[r], peers, WORLD_CALL, K, n, crop, intr, fr, bound)
            u = e["union"]                                       # seeds here: own first, then the peers in rank order
            if u.value > e["own_max"]:
                assert u.seed >= 1
                seen["greater"] += 1
                seen["first"] += u.seed == 1
                seen["last"] += u.seed == w - 1
                seen["second_block"] += u.i >= 256
        assert len({e["union"].value.tobytes() for e in exp.values()}) == 1
        cases.append((w, n, K, seeds, fr, exp))
    assert all(v > 0 for v in seen.values()), seen
    return cases


def not_counted_case(frames, crop, intr, bound, world=4, n=40, K=3, call=5):
    """Peer-exclusive pixels that must not reach the header: one with a depth beyond its ray's exit distance (larger than every
    kept depth, but not kept), one with depth 0, one with a negative depth.  -> seeds, frames, the reference of rank 0 -- which
    must ignore all three: its union maximum is the one of the unedited frames."""
    seeds = seeds_for(4242, world)
    frames = frames_with(frames, K)
    before = union_max(seeds, call, K, n, crop, intr, frames, bound)
    values = []
    for peer, value in ((1, None), (2, 0.0), (world - 1, -3.0)):
        k, i, index, t = exclusive_rays(seeds, call, K, n, crop, intr, frames, bound, peer)[0]
        value = np.float32(2.0 * t + 10.0) if value is None else value
        assert value <= 0 or (value > t and value > before.value)
        frames = set_depth(frames, k, crop, index, float(value))
        values.append(value)
    exp = expected_launch(seeds[0], seeds[1:], call, K, n, crop, intr, frames, bound)
    assert exp["union"].value == before.value > 0 and values[0] > before.value
    return seeds, frames, exp, call


def far_bound(bound):
    """a bound no ray of a camera inside ``bound`` reaches: every ray leaves it at a negative distance, so none is kept"""
    return torch.as_tensor(bound, dtype=torch.float64) + 50.0
