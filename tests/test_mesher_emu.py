"""CPU tests of the mesh-extraction kernels (nice_slam_amd/csrc/nsr_kernels.h, "Mesh extraction") and of the host glue in
nice_slam_amd/mesher.py, executed under the emulator (tests/emu/) at small sizes, against the numpy restatements of
tests/mesh_reference.py, scipy's connected components, and a golden minted from the reference's Mesher
(tests/golden/make_golden_mesher.py)."""
import os

import numpy as np
import pytest
import torch

import mesh_reference as MR
from emu_harness import emu_lib, ptr
from nice_slam_amd.engine import Engine, c_doubles
from nice_slam_amd.mesher import face_components, keep_components, marching_cubes, point_masks_raw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesher_masks.npz")


@pytest.fixture(scope="module")
def E():
    return Engine(emu_lib(), "cpu")


def emu(E, fn, *args):
    """one of the mesher's functions on host tensors under the emulator engine; numpy results"""
    out = fn(*(torch.from_numpy(a) if isinstance(a, np.ndarray) else a for a in args), engine=E)
    return tuple(t.numpy() for t in out) if isinstance(out, tuple) else out.numpy()


def mc(E, vol, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    return emu(E, marching_cubes, vol, level, spacing, origin)


def lattice(n, shift=0.3):
    g = np.arange(n, dtype=np.float64) - n / 2 + shift
    return np.meshgrid(g, g, g, indexing="ij")


def sphere(n=32, r=12.0):
    X, Y, Z = lattice(n)
    return (r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)


def torus(n=32, R=9.0, r=4.0):
    X, Y, Z = lattice(n)
    return (r - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - R) ** 2 + Z ** 2)).astype(np.float32)


def noise(seed, shape=(14, 15, 16)):
    v = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    v[0] = v[-1] = -5
    v[:, 0] = v[:, -1] = -5
    v[:, :, 0] = v[:, :, -1] = -5
    return v


def assert_same(got, ref):
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape
    assert np.array_equal(got[0], ref[0])            # bit for bit (fp64)
    assert np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("name", ["sphere", "torus", "noise0", "noise1", "plane", "empty"])
def test_mc_matches_restatement(E, name):
    spacing, origin, level = (0.5, 0.25, 0.125), (-1.5, 2.0, 0.75), 0.0
    if name == "sphere":
        vol = sphere()
    elif name == "torus":
        vol = torus()
    elif name.startswith("noise"):
        vol, level = noise(int(name[-1])), 0.1
    elif name == "plane":
        X, Y, Z = lattice(12, 0.0)
        vol = (Y - 1.0).astype(np.float32)            # exactly 0 on the lattice plane y = 1
        vol[:, :, 5] += 0.5
    else:
        vol = np.full((9, 10, 11), -1.0, np.float32)
    got = mc(E, vol, level, spacing, origin)
    ref = MR.marching_cubes(vol, level, spacing, origin)
    assert_same(got, ref)
    if name == "empty":
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    else:
        assert len(got[1]) > 0


@pytest.mark.parametrize("seed", range(4))
def test_mc_noise_is_crack_free(E, seed):
    v, f = mc(E, noise(seed), 0.0)
    assert len(f) > 1000
    assert set(MR.edge_use_counts(f).tolist()) == {2}     # every mesh edge of the closed surface: exactly two faces


def test_mc_table_properties():
    tab = MR.mc_table()
    assert max(len(t) for t in tab) == 5 and tab[0] == [] and tab[255] == []
    # complementary cases cut the same edges
    for k in range(256):
        assert {e for t in tab[k] for e in t} == {e for t in tab[255 - k] for e in t}


def test_mc_topology_volume_orientation(E):
    r = 12.0
    v, f = mc(E, sphere(32, r))
    assert MR.euler_characteristic(v, f) == 2
    vol = MR.signed_volume(v, f)
    assert vol > 0                                           # normals point toward decreasing field (outward)
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1) < 0.01
    v, f = mc(E, torus())
    assert MR.euler_characteristic(v, f) == 0 and MR.signed_volume(v, f) > 0


def test_mc_sphere_volume_at_r20():
    r = 20.0
    X, Y, Z = lattice(44)
    vol = (r - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)
    v, f = MR.marching_cubes(vol)                          # (44^3 under the emulator is slow; the kernel equals this above)
    assert abs(MR.signed_volume(v, f) / (4.0 / 3.0 * np.pi * r ** 3) - 1) < 0.01


def test_mc_vertices_on_straddling_edges(E):
    vol = noise(7, (9, 10, 11))
    level = np.float32(0.2)
    sp, org = np.array([0.5, 0.25, 2.0]), np.array([1.0, -2.0, 3.0])
    v, f = mc(E, vol, level, sp, org)
    g = (v - org) / sp
    fl = np.floor(g + 1e-9)
    frac = g - fl
    ax = np.argmax(frac > 1e-12, axis=1)
    assert ((frac > 1e-12).sum(1) <= 1).all()
    idx = fl.astype(np.int64)
    a = vol[idx[:, 0], idx[:, 1], idx[:, 2]]
    step = np.eye(3, dtype=np.int64)[ax]
    b = vol[idx[:, 0] + step[:, 0], idx[:, 1] + step[:, 1], idx[:, 2] + step[:, 2]]
    assert ((a > level) != (b > level)).all()
    t = (level - a) / (b - a)
    assert np.allclose(frac[np.arange(len(v)), ax], t, atol=1e-6)


def test_mc_abi_errors():
    lib = emu_lib()
    vol = np.zeros((4, 4, 4), np.float32)
    ws = np.zeros(lib.nsr_mc_workspace_bytes(4, 4, 4), np.uint8)
    counts = np.zeros(2, np.int64)
    assert lib.nsr_mc_workspace_bytes(1, 4, 4) == -1
    assert lib.nsr_mc_count(ptr(vol), 4, 1, 4, 0.0, ptr(ws), ptr(counts), None) != 0
    assert b"at least 2" in lib.nsr_last_error()
    assert lib.nsr_mc_count(None, 4, 4, 4, 0.0, ptr(ws), ptr(counts), None) != 0
    assert lib.nsr_mc_count(ptr(vol), 4, 4, 4, 0.0, ptr(ws), None, None) != 0
    out_v, out_f = np.zeros((1, 3)), np.zeros((1, 3), np.int32)
    o, sp = c_doubles((0, 0, 0)), c_doubles((1, 1, 1))
    assert lib.nsr_mc_emit(ptr(vol), 4, 4, 4, 0.0, o, sp, ptr(ws), 1, 1 << 30, ptr(out_v), ptr(out_f), None) != 0
    assert b"int32" in lib.nsr_last_error()
    assert lib.nsr_mc_emit(ptr(vol), 4, 4, 4, 0.0, o, sp, ptr(ws), 1 << 31, 1, ptr(out_v), ptr(out_f), None) != 0
    assert lib.nsr_mc_emit(ptr(vol), 4, 4, 4, 0.0, o, sp, ptr(ws), 1, 1, None, ptr(out_f), None) != 0
    assert lib.nsr_point_masks(None, 10, 5, 0, 1, None, None, None, 8, 8, 1.0, 1.0, 1.0, 1.0, None, None, None) != 0
    assert lib.nsr_point_masks(ptr(vol), 10, 5, 3, 0, None, None, None, 8, 8, 1.0, 1.0, 1.0, 1.0, None, ptr(ws), None) != 0
    assert lib.nsr_face_areas(None, None, 3, None, None) != 0
    assert lib.nsr_cc_init(-1, None, None, None) != 0


# ---- point masks ----

def masks(E, points, c2ws, depths, H, W, fx, fy, cx, cy, mode, chunk):
    return emu(E, point_masks_raw, points, c2ws, [torch.from_numpy(d) for d in depths], H, W, fx, fy, cx, cy, mode, chunk)


@pytest.fixture(scope="module")
def mask_golden():
    if not os.path.exists(GOLDEN):
        pytest.fail("tests/golden/mesher_masks.npz missing (tests/golden/make_golden_mesher.py)")
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_point_masks_match_reference_golden(E, mask_golden, mode):
    g = mask_golden
    H, W = int(g["H"]), int(g["W"])
    fx, fy, cx, cy = (float(x) for x in g["intr"])
    pts, chunk = g["points"], int(g["chunk"])
    if mode == 0:
        c2ws, depths = list(g["all_c2w"]), []
    else:
        c2ws, depths = list(g["kf_c2w"]), list(g["kf_depth"])
    want = g[f"mask_mode{mode}"]
    got = masks(E, pts, c2ws, depths, H, W, fx, fy, cx, cy, mode, chunk)
    ref = MR.point_masks(pts, c2ws, depths, H, W, fx, fy, cx, cy, mode, chunk)
    assert np.array_equal(got, ref)
    assert np.array_equal(got, want)
    assert (want == 1).sum() > 20 and (want == 2).sum() > 20 and (want == 0).sum() > 20


def test_point_masks_chunk_max_matters(mask_golden):
    """the forecast cut of the depth-test branch uses the maximum over the CHUNK: with one chunk for all points the masks differ"""
    g = mask_golden
    H, W = int(g["H"]), int(g["W"])
    fx, fy, cx, cy = (float(x) for x in g["intr"])
    args = (g["points"], list(g["kf_c2w"]), list(g["kf_depth"]), H, W, fx, fy, cx, cy, 2)
    assert not np.array_equal(MR.point_masks(*args, len(g["points"])), g["mask_mode2"])


@pytest.mark.parametrize("chunk", [64, 200, 5000])
def test_point_masks_wave_reduced_chunk_max(E, mask_golden, chunk):
    """chunks of >= 64 points: waves that lie in one chunk reduce the sampled depths before the atomic maximum"""
    g = mask_golden
    H, W = int(g["H"]), int(g["W"])
    fx, fy, cx, cy = (float(x) for x in g["intr"])
    args = (g["points"], list(g["kf_c2w"]), list(g["kf_depth"]), H, W, fx, fy, cx, cy, 2, chunk)
    assert np.array_equal(masks(E, *args), MR.point_masks(*args))


def test_grid_uniform_matches_reference_golden(mask_golden):
    pts, _ = MR.grid_uniform(mask_golden["mc_bound"], int(mask_golden["grid_res"]))
    assert np.array_equal(pts, mask_golden["grid_points"])


# ---- connected components ----

def components(E, verts, faces):
    """-> per-face label (largest face index of the component), per-face area, per-component area (by label order), component
    labels; the per-face areas from the same mesh with every face split off into a component of its own"""
    label, seg_area, first, _ = emu(E, face_components, verts, faces)
    split = np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)
    area = emu(E, face_components, verts[faces].reshape(-1, 3), split)[1]
    return label, area, seg_area, label[first]


def two_spheres_and_blob():
    n = 28
    X, Y, Z = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), np.arange(12, dtype=np.float64), indexing="ij")
    f = np.maximum(np.maximum(4.5 - np.sqrt((X - 7) ** 2 + (Y - 7) ** 2 + (Z - 5.5) ** 2),
                              4.0 - np.sqrt((X - 19) ** 2 + (Y - 18) ** 2 + (Z - 5.5) ** 2)),
                   1.2 - np.sqrt((X - 20) ** 2 + (Y - 5) ** 2 + (Z - 5.5) ** 2))
    return MR.marching_cubes(f.astype(np.float32))


def test_components_match_scipy(E):
    v, f = two_spheres_and_blob()
    label, area, seg_area, seg_label = components(E, v, f)
    ref = MR.face_adjacency_components(f)
    assert len(np.unique(ref)) == 3 and len(seg_label) == 3
    # the same partition
    pairs = {(a, b) for a, b in zip(label.tolist(), ref.tolist())}
    assert len(pairs) == 3
    # a component's label is its largest face index
    for lab in seg_label:
        assert lab == np.nonzero(label == lab)[0].max()
    assert np.allclose(area, MR.face_areas(v, f), rtol=1e-12, atol=0)
    for s, lab in enumerate(seg_label):
        assert np.isclose(seg_area[s], area[label == lab].sum(), rtol=1e-12)


def test_components_vertex_touch_stays_split(E):
    # two triangle fans that share only vertex 0
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [-1, 0, 0], [0, -1, 0], [-1, -1, 0]], np.float64)
    f = np.array([[0, 1, 2], [1, 3, 2], [0, 4, 5], [4, 6, 5]], np.int32)
    label, *_ = components(E, v, f)
    assert label[0] == label[1] and label[2] == label[3] and label[0] != label[2]
    assert len(np.unique(MR.face_adjacency_components(f))) == 2


def test_component_keep_rules(E):
    v, f = two_spheres_and_blob()
    ref = MR.face_adjacency_components(f)
    ref_area = np.array([MR.face_areas(v, f)[ref == c].sum() for c in range(ref.max() + 1)])

    def kept(largest, min_area):
        """the corners of the faces keep_components keeps, in face order (its vertices are compacted, so compare positions)"""
        kv, kf = emu(E, keep_components, v, f, largest, min_area)
        assert len(np.unique(kf)) == len(kv)
        return kv[kf]

    keep_big = ref == np.argmax(ref_area)
    assert np.array_equal(kept(True, 0), v[f[keep_big]])
    thr = np.sort(ref_area)[0] * 1.5                # drops the blob only
    keep_thr = ref_area[ref] > thr
    assert np.array_equal(kept(False, thr), v[f[keep_thr]])
    assert keep_thr.sum() < len(f) and keep_big.sum() < keep_thr.sum()


# ---- PLY ----

def test_ply_roundtrip(tmp_path):
    from nice_slam_amd.ply import read_mesh, write_ply
    v, f = two_spheres_and_blob()
    col = (np.arange(len(v) * 3) % 256).astype(np.uint8).reshape(-1, 3)
    p = str(tmp_path / "m.ply")
    write_ply(p, v, f, col)
    rv, rf, rc = read_mesh(p, colors=True)
    assert np.array_equal(rv, v.astype(np.float32)) and np.array_equal(rf, f)
    assert np.array_equal(rc[:, :3], col) and (rc[:, 3] == 255).all()
    with open(p, "rb") as fh:
        assert fh.read(60).startswith(b"ply\nformat binary_little_endian 1.0\n")
    write_ply(p, v, f)
    rv, rf, rc = read_mesh(p, colors=True)
    assert rc is None and np.array_equal(rf, f)
