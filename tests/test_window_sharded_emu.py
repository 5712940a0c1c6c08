"""CPU: the window kernel as one rank of a ray-sharded iteration (nsr_get_samples_window_sharded, get_samples_window_kernel with
n_peers > 0) on the emulator, against tests/window_reference.py: the peer block indexing, the last-block hand-off count over
the peers' blocks, the fill blocks behind them, the call counter's high word and the refusals -- at one to fifteen peers."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import window_reference as wr
from test_emu_parity import _window_case


@pytest.fixture(scope="module")
def emu():
    if not (os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("clang++")):
        pytest.skip("no host clang++ for the emulator build")
    from emu_harness import emu_lib
    return emu_lib()


class _Case:
    """the frames of _window_case() as the reference and the C ABI want them"""

    def __init__(self):
        sc, frames, _, crop = _window_case()
        H, W, fx, fy, cx, cy = sc["intr"]
        self.W, self.crop, self.intr, self.bound, self.frames = W, crop, (fx, fy, cx, cy), sc["bound"], frames


@pytest.fixture(scope="module")
def case():
    return _Case()


def _launch(emu, case, frames, own_seed, call, peers, K, n, zero_n=0, bound=None, state=None, n_peers=None, null_seeds=False,
            header_offset=0, fused_no_peers=False):
    """One launch on host buffers -> (return code, the buffers as wr.check_launch reads them).  ``state``: an existing state array to
    launch from (default: a fresh [own_seed, call, 0, 0])."""
    from emu_harness import ptr
    from nice_slam_amd import _capi
    N = max(K, 0) * max(n, 0)
    fr = (_capi.NsrFrame * max(1, len(frames)))()
    hold = []
    for k, (c2w, d, col) in enumerate(frames):
        arrs = [np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (d, col, c2w)]
        hold += arrs
        fr[k].depth, fr[k].color, fr[k].c2w, fr[k].c2w_stride = arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, 4
    b = case.bound if bound is None else bound
    lo, hi = (C.c_double * 3)(*b[:, 0].tolist()), (C.c_double * 3)(*b[:, 1].tolist())
    got = {name: np.full((N * wr.WIDTH[name] + wr.GUARD,), fill, np.int64 if name == "indices" else np.uint8 if name == "keep" else np.float32)
           for name, fill in wr.PREFILL.items()}
    raw = np.full((4 + header_offset + 4 + zero_n + wr.GUARD,), np.nan, np.float32)
    base = (-(raw.ctypes.data // 4)) % 4                         # floats up to the next 16-byte boundary
    Z = raw[base + header_offset:base + header_offset + 4 + zero_n + wr.GUARD]      # header | span | guard (header_offset: misaligned)
    Z[-wr.GUARD:] = wr.SPAN_GUARD
    st = np.array([own_seed, call, 0, 0], dtype=np.uint64) if state is None else state
    seeds = None if (null_seeds or not peers) else (C.c_uint64 * len(peers))(*peers)
    tail = (K, n, *case.crop, case.W, *case.intr, fr, ptr(got["rays_o"]), ptr(got["rays_d"]), ptr(got["gt_depth"]), ptr(got["gt_color"]),
            lo, hi, ptr(got["keep"]), ptr(Z), ptr(Z[4:]) if zero_n else None, zero_n, None)
    if fused_no_peers:
        rc = emu.nsr_get_samples_window_fused(None, ptr(got["indices"]), ptr(st), *tail)
    else:
        rc = emu.nsr_get_samples_window_sharded(ptr(got["indices"]), ptr(st), seeds, len(peers) if n_peers is None else n_peers, *tail)
    got["Z"], got["state"] = Z, st.copy()
    return rc, got


def _expected(case, frames, own, peers, call, K, n, bound=None):
    return wr.expected_launch(own, peers, call, K, n, case.crop, case.intr, frames, case.bound if bound is None else bound)


@pytest.mark.parametrize("n_peers,n,K", wr.GEOMETRIES)
def test_geometry_sweep(emu, case, n_peers, n, K):
    """own indices = the reference draw, own rays / depth / colour / mask bit-equal to the reference on them, nothing written behind
    any output (the peers' draws write nothing at all), header {0, 0, union maximum, 0} bit-equal, state [seed, call + 1, 0, 0],
    the span zero to the float -- per geometry with seeds of its own, from call counter 5, at three span lengths."""
    seeds, frames, exp = wr.geometry_case(case.frames, case.crop, case.intr, case.bound, n_peers, n, K)
    for zero_n in wr.ZERO_SPANS:
        rc, got = _launch(emu, case, frames, seeds[0], 5, seeds[1:], K, n, zero_n)
        assert rc == 0
        wr.check_launch(got, exp, K * n, zero_n, seeds[0], 6)


@pytest.fixture(scope="module")
def worlds(case):
    return wr.world_cases(case.frames, case.crop, case.intr, case.bound)       # asserts the discriminating situations (reference only)


def test_every_rank_of_one_world_gets_the_same_header(emu, case, worlds):
    """W launches, one as each rank (own seed = that rank's, the others as peers in rank order), all from one call counter: W
    bit-identical headers equal to the reference -- in worlds of 2, 3, 8 and 16 ranks whose maximum is held by a first peer, a
    last peer and a peer's second x-block (window_reference.world_cases asserts that on the reference alone)."""
    assert sorted({c[0] for c in worlds}) == [2, 3, 8, 16]
    for w, n, K, seeds, frames, exp in worlds:
        headers = []
        for r in range(w):
            rc, got = _launch(emu, case, frames, seeds[r], wr.WORLD_CALL, [s for q, s in enumerate(seeds) if q != r], K, n, 5)
            assert rc == 0
            wr.check_launch(got, exp[r], K * n, 5, seeds[r], wr.WORLD_CALL + 1)
            headers.append(got["Z"][:4].tobytes())
        assert len(set(headers)) == 1, (w, n, K)


def test_rays_that_must_not_count(emu, case):
    """a peer's ray beyond its exit distance (deeper than every kept ray), a peer's ray of depth 0 and one of negative depth stay
    out of the header; with a bound no ray reaches nothing is kept on any rank and the maximum is 0.0"""
    seeds, frames, exp, call = wr.not_counted_case(case.frames, case.crop, case.intr, case.bound)
    rc, got = _launch(emu, case, frames, seeds[0], call, seeds[1:], 3, 40, 5)
    assert rc == 0
    wr.check_launch(got, exp, 120, 5, seeds[0], call + 1)
    far = wr.far_bound(case.bound)
    exp = _expected(case, frames, seeds[0], seeds[1:], call, 3, 40, bound=far)
    assert exp["union"].value == 0.0 and not exp["keep"].any() and exp["union"].seed is None
    rc, got = _launch(emu, case, frames, seeds[0], call, seeds[1:], 3, 40, 5, bound=far)
    assert rc == 0
    wr.check_launch(got, exp, 120, 5, seeds[0], call + 1)
    assert got["Z"][2].tobytes() == np.float32(0.0).tobytes()


@pytest.mark.parametrize("call", [5, 2 ** 32 + 5])
def test_peers_follow_the_call_counter(emu, case, call):
    """two launches in a row from one state: the second header is the union maximum at call + 1; from call = 2^32 + 5 the high
    word of the counter reaches the draw of the rank and of its peers"""
    K, n = 3, 300
    seeds = wr.seeds_for(77, 4)
    frames = wr.frames_with(case.frames, K)
    crop_pixels = (case.crop[1] - case.crop[0]) * (case.crop[3] - case.crop[2])
    if call >> 32:                                               # (the reference's draw itself depends on the high word)
        assert not np.array_equal(wr.draw(seeds[1], call, K, n, crop_pixels), wr.draw(seeds[1], call & 0xFFFFFFFF, K, n, crop_pixels))
    state = np.array([seeds[0], call, 0, 0], dtype=np.uint64)
    values = []
    for c in (call, call + 1):
        exp = _expected(case, frames, seeds[0], seeds[1:], c, K, n)
        rc, got = _launch(emu, case, frames, seeds[0], c, seeds[1:], K, n, 5, state=state)
        assert rc == 0
        wr.check_launch(got, exp, K * n, 5, seeds[0], c + 1)
        values.append(exp["indices"])
    assert (values[0] != values[1]).mean() > 0.9


def test_refusals_write_nothing(emu, case):
    K, n = 3, 40
    seeds = wr.seeds_for(78, 17)
    frames = wr.frames_with(case.frames, K)
    for what, kw, peers in (("16 peers", {}, seeds[1:17]), ("-1 peers", {"n_peers": -1}, seeds[1:4]),
                            ("null seeds", {"n_peers": 3, "null_seeds": True}, seeds[1:4]), ("header alignment", {"header_offset": 1}, seeds[1:4]),
                            ("K = 0", {"K": 0}, seeds[1:4]), ("n = 0", {"n": 0}, seeds[1:4])):
        kw = dict(kw)
        rc, got = _launch(emu, case, frames, seeds[0], 5, peers, kw.pop("K", K), kw.pop("n", n), 5, **kw)
        assert rc != 0, what
        assert wr.untouched(got), what
        assert got["state"].tolist() == [seeds[0], 5, 0, 0], what


def test_no_peers_is_the_fused_launch_with_a_draw(emu, case):
    K, n = 3, 300
    seed = wr.seeds_for(79, 1)[0]
    frames = wr.frames_with(case.frames, K)
    rc_a, a = _launch(emu, case, frames, seed, 5, [], K, n, 70001)
    rc_b, b = _launch(emu, case, frames, seed, 5, [], K, n, 70001, fused_no_peers=True)
    assert rc_a == 0 and rc_b == 0
    for name in a:
        assert wr.same(a[name], b[name]), name
    wr.check_launch(a, _expected(case, frames, seed, [], 5, K, n), K * n, 70001, seed, 6)
