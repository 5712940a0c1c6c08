"""GPU, one process: the window kernel as one rank of a ray-sharded iteration (nsr_get_samples_window_sharded) at one to fifteen
peers against tests/window_reference.py (bit for bit: the header's maximum is a selection), under back-to-back launches and graph
replay -- and a simulated world of 3, 8 and 16 ranks through ``mapping_loss(draw_state=, peer_seeds=)``: the ranks' summed losses
and gradients against ONE call on the union batch (tests/test_hip_dist.py's two-rank assertion without processes)."""
import ctypes as C

import numpy as np
import pytest
import torch

import window_reference as wr
from scene_util import build_product, make_scene, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Case:
    def __init__(self):
        sc = make_scene(seed=83, n_rays=8, small=True)
        H, W, fx, fy, cx, cy = sc["intr"]
        g = torch.Generator().manual_seed(17)
        self.frames = []
        for k in range(3):
            c2w = sc["c2w"].clone()
            c2w[:3, 3] += 0.02 * k
            self.frames.append((c2w[:3].contiguous() if k % 2 else c2w, sc["depth_img"] * (1.0 + 0.03 * k), torch.rand((H, W, 3), generator=g)))
        self.W, self.crop, self.intr, self.bound = W, (4, H - 4, 5, W - 5), (fx, fy, cx, cy), sc["bound"]


@pytest.fixture(scope="module")
def case():
    return _Case()


class _Launch:
    """The device buffers of one launch (pre-filled, wr.GUARD elements behind every output) and its enqueue on the current stream"""

    def __init__(self, case, frames, K, n, zero_n, bound=None):
        from nice_slam_amd import mapping
        dev = torch.device(DEV)
        self.case, self.K, self.n, self.zero_n = case, K, n, zero_n
        N = K * n
        self.buf = {name: torch.full((N * wr.WIDTH[name] + wr.GUARD,), fill, device=dev,
                                     dtype=torch.int64 if name == "indices" else torch.uint8 if name == "keep" else torch.float32)
                    for name, fill in wr.PREFILL.items()}
        self.Z = torch.full((4 + zero_n + wr.GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.Z[-wr.GUARD:] = wr.SPAN_GUARD
        assert self.Z.data_ptr() % 16 == 0
        dfr = [tuple(t.to(dev) for t in f) for f in frames]
        self.fr, self.hold = mapping._frames_block([f[0] for f in dfr], [f[1] for f in dfr], [f[2] for f in dfr], dev)
        self.lo, self.hi = mapping._bound_arrays(case.bound if bound is None else bound)

    def enqueue(self, state, peers):
        from nice_slam_amd import _capi
        from nice_slam_amd.common import _stream
        lib, b, c = _capi.get_lib(), self.buf, self.case
        seeds = (C.c_uint64 * len(peers))(*peers) if peers else None
        lib.check(lib.nsr_get_samples_window_sharded(
            b["indices"].data_ptr(), state.data_ptr(), seeds, len(peers), self.K, self.n, *c.crop, c.W, *c.intr, self.fr,
            b["rays_o"].data_ptr(), b["rays_d"].data_ptr(), b["gt_depth"].data_ptr(), b["gt_color"].data_ptr(), self.lo, self.hi,
            b["keep"].data_ptr(), self.Z.data_ptr(), self.Z.data_ptr() + 16 if self.zero_n else None, self.zero_n,
            _stream(torch.device(DEV))), "nsr_get_samples_window_sharded")

    def read(self, state):
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.buf.items()}
        got["Z"], got["state"] = self.Z.cpu().numpy(), state.cpu().numpy().astype(np.uint64)
        return got


def _state(seed, call):
    return torch.tensor([wr.M64 & seed, call, 0, 0], dtype=torch.int64, device=DEV)


def _run(case, frames, own, peers, call, K, n, zero_n, exp, bound=None):
    la = _Launch(case, frames, K, n, zero_n, bound)
    st = _state(own, call)
    la.enqueue(st, peers)
    got = la.read(st)
    wr.check_launch(got, exp, K * n, zero_n, own, call + 1)
    return got


def _expected(case, frames, own, peers, call, K, n, bound=None):
    return wr.expected_launch(own, peers, call, K, n, case.crop, case.intr, frames, case.bound if bound is None else bound)


@pytest.mark.parametrize("n_peers,n,K", wr.GEOMETRIES)
def test_geometry_sweep(case, n_peers, n, K):
    """tests/test_window_sharded_emu.py::test_geometry_sweep on the hardware"""
    seeds, frames, exp = wr.geometry_case(case.frames, case.crop, case.intr, case.bound, n_peers, n, K)
    for zero_n in wr.ZERO_SPANS:
        _run(case, frames, seeds[0], seeds[1:], 5, K, n, zero_n, exp)


def test_every_rank_of_one_world_gets_the_same_header(case):
    worlds = wr.world_cases(case.frames, case.crop, case.intr, case.bound)     # asserts the discriminating situations (reference only)
    assert sorted({c[0] for c in worlds}) == [2, 3, 8, 16]
    for w, n, K, seeds, frames, exp in worlds:
        headers = [_run(case, frames, seeds[r], [s for q, s in enumerate(seeds) if q != r], wr.WORLD_CALL, K, n, 5, exp[r])["Z"][:4].tobytes()
                   for r in range(w)]
        assert len(set(headers)) == 1, (w, n, K)


def test_rays_that_must_not_count(case):
    seeds, frames, exp, call = wr.not_counted_case(case.frames, case.crop, case.intr, case.bound)
    _run(case, frames, seeds[0], seeds[1:], call, 3, 40, 5, exp)
    far = wr.far_bound(case.bound)
    exp = _expected(case, frames, seeds[0], seeds[1:], call, 3, 40, bound=far)
    assert exp["union"].value == 0.0 and not exp["keep"].any()
    got = _run(case, frames, seeds[0], seeds[1:], call, 3, 40, 5, exp, bound=far)
    assert got["Z"][2].tobytes() == np.float32(0.0).tobytes()


@pytest.mark.parametrize("call", [5, 2 ** 32 + 5])
def test_peers_follow_the_call_counter(case, call):
    """two launches from one state, each read back before the next; call = 2^32 + 5: the counter's high word"""
    K, n = 3, 300
    seeds = wr.seeds_for(77, 4)
    frames = wr.frames_with(case.frames, K)
    st = _state(seeds[0], call)
    for c in (call, call + 1):
        la = _Launch(case, frames, K, n, 5)
        la.enqueue(st, seeds[1:])
        wr.check_launch(la.read(st), _expected(case, frames, seeds[0], seeds[1:], c, K, n), K * n, 5, seeds[0], c + 1)


def test_fill_blocks_behind_eight_ranks_draw_blocks(case):
    """a 48 MB span at seven peers: the 2048 fill blocks start behind 8 x 2 x 3 draw blocks"""
    K, n, zero_n = 3, 300, 12 * 1024 * 1024 + 3
    seeds = wr.seeds_for(80, 8)
    frames = wr.frames_with(case.frames, K)
    _run(case, frames, seeds[0], seeds[1:], 5, K, n, zero_n, _expected(case, frames, seeds[0], seeds[1:], 5, K, n))


def test_back_to_back_launches_on_one_stream(case):
    """no synchronisation between two launches: the second finds the hand-off words as the first left them"""
    K, n = 3, 300
    seeds = wr.seeds_for(81, 4)
    frames = wr.frames_with(case.frames, K)
    exps = [_expected(case, frames, seeds[0], seeds[1:], c, K, n) for c in (5, 6)]
    las = [_Launch(case, frames, K, n, 70001) for _ in range(2)]
    st = _state(seeds[0], 5)
    torch.cuda.synchronize()
    for la in las:
        la.enqueue(st, seeds[1:])
    for la, exp in zip(las, exps):
        wr.check_launch(la.read(st), exp, K * n, 70001, seeds[0], 7)
    assert exps[0]["union"].value > 0


def test_graph_replay_advances_the_peers_with_the_rank(case):
    """one captured launch (4 ranks, n = 300, K = 3; a single stream, no parallel branches) replayed three times: indices and
    header are the reference's at each replay's call number"""
    K, n, call = 3, 300, 9
    seeds = wr.seeds_for(82, 4)
    frames = wr.frames_with(case.frames, K)
    la = _Launch(case, frames, K, n, 70001)
    st = _state(seeds[0], call)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        la.enqueue(st, seeds[1:])
    torch.cuda.synchronize()
    assert st.tolist() == [seeds[0], call, 0, 0]                 # the capture itself drew nothing
    for rep in range(3):
        g.replay()
        wr.check_launch(la.read(st), _expected(case, frames, seeds[0], seeds[1:], call + rep, K, n), K * n, 70001, seeds[0], call + rep + 1)


# ----------------------------------------------------------------------------------------------------------------------
# a simulated world through the product's Python surface
# ----------------------------------------------------------------------------------------------------------------------
K_FR, M_PIX = 3, 25


def _map_frames(sc, dev):
    H, W = sc["intr"][:2]
    g = torch.Generator().manual_seed(33)
    out = []
    for k in range(K_FR):
        c2w = sc["c2w"].clone()
        c2w[:3, 3] += 0.02 * k
        out.append((c2w.to(dev).requires_grad_(True), (sc["depth_img"] * (1.0 + 0.05 * k)).to(dev), torch.rand((H, W, 3), generator=g).to(dev)))
    return out


@pytest.fixture(scope="module")
def product():
    sc = make_scene(seed=5, n_rays=8, small=True)
    return (sc, *build_product(sc, DEV))


def _iteration(product, stage, **kw):
    """one mapping iteration on fresh leaves -> loss, {name: gradient} (fp64 on the host), the `out` dict"""
    import nice_slam_amd as nsa
    sc, renderer, dec, grids = product
    frames = _map_frames(sc, DEV)
    c = {k: v.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for k, v in grids.items()}
    for p in dec.parameters():
        p.requires_grad_(True)
        p.grad = None
    info = {}
    loss = nsa.mapping_loss(renderer, c, dec, frames, kw.pop("pixs"), stage, out=info, **kw)
    loss.backward()
    torch.cuda.synchronize()
    grads = {"grid/" + k: v.grad.double().cpu().numpy() for k, v in c.items() if v.grad is not None}
    grads.update({"dparam/" + k: p.grad.double().cpu().numpy().copy() for k, p in dec.named_parameters() if p.grad is not None})
    grads.update({"pose/%d" % i: f[0].grad.double().cpu().numpy() for i, f in enumerate(frames)})
    return float(loss.detach()), grads, info


GATES = {"grid": 2e-6, "dparam": 2e-5, "pose": 1e-4}             # tests/test_hip_dist.py::test_two_ranks_sharded_fused_mapping's own


@pytest.mark.parametrize("world", [3, 8, 16])
def test_simulated_world_sums_to_one_gpu_on_the_union_batch(product, world):
    """Every rank of a world of 3 / 8 / 16 as one call of mapping_loss with that rank's draw state and its peers' seeds (what
    ShardedMapping.mapping_loss passes; rank_seed needs no process group, so the object is built with group=None and
    torch.distributed is never initialised): bit-identical depth caps, different pixels per rank, and the fp64 sums of the ranks'
    losses and gradients equal to one call on the frame-major union of their draws."""
    from nice_slam_amd.parallel import ShardedMapping
    sc, renderer = product[0], product[1]
    sh = ShardedMapping(renderer, group=None, seed=3)
    seeds = [sh.rank_seed(r) for r in range(world)]
    assert len(set(seeds)) == world
    for stage, call in (("color", 4), ("fine", 5)):
        ranks = []
        for r in range(world):
            state = torch.tensor([seeds[r], call, 0, 0], dtype=torch.int64, device=DEV)
            peers = [seeds[q] for q in range(world) if q != r]   # ShardedMapping.peer_seeds(): every other rank, in rank order
            loss, grads, info = _iteration(product, stage, pixs=M_PIX, draw_state=state, peer_seeds=peers)
            assert state.tolist() == [seeds[r], call + 1, 0, 0]
            ranks.append((loss, grads, info["indices"].cpu().reshape(K_FR, M_PIX), info["kept_max"].cpu().numpy().tobytes()))
        assert len({r[3] for r in ranks}) == 1, "the ranks disagree on the depth cap"
        assert np.frombuffer(ranks[0][3], np.float32)[0] > 0
        H, W = sc["intr"][:2]
        for r, rk in enumerate(ranks):
            assert np.array_equal(rk[2].numpy().reshape(-1), wr.draw(seeds[r], call, K_FR, M_PIX, H * W)), r
            assert all(not torch.equal(rk[2], other[2]) for other in ranks[:r]), "two ranks drew the same pixels"
        idx = torch.cat([rk[2] for rk in ranks], 1).reshape(-1)   # frame-major: [frame][rank 0's draw | rank 1's draw | ...]
        loss, ref, info = _iteration(product, stage, pixs=world * M_PIX, indices=idx)
        assert info["kept_max"].cpu().numpy().tobytes() == ranks[0][3]
        total = sum(rk[0] for rk in ranks)
        errs = {k: rel_err(sum(rk[1][k] for rk in ranks), v) for k, v in ref.items()}
        print(f"world {world} {stage}: loss {abs(total - loss) / abs(loss):.2e}; " +
              "; ".join(f"{kind} {max(e for k, e in errs.items() if k.startswith(kind)):.2e}" for kind in GATES))
        assert set(ranks[0][1]) == set(ref) and any(k.startswith("pose/") for k in ref) and any(k.startswith("dparam/") for k in ref)
        assert abs(total - loss) < 1e-5 * abs(loss), (stage, total, loss)
        for k, e in errs.items():
            assert e < GATES[k.split("/")[0]], (world, stage, k, e)
