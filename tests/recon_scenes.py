"""TEST INFRASTRUCTURE: analytic scenes for the reconstruction-evaluation tests and tools/recon_eval_timing.py -- a room
(walls, floor, ceiling, a table, two spheres) as a dense fp32 field with its exact surface sampled analytically, a bumpy
closed object for ICP, and clouds on the room's surface."""
import numpy as np

ROOM_LO, ROOM_HI = np.array([0.0, 0.0, 0.0]), np.array([5.0, 4.0, 3.0])
TABLE_C, TABLE_H = np.array([2.0, 1.5, 0.75]), np.array([0.8, 0.5, 0.35])       # centre, half extents
SPHERES = ((np.array([3.8, 2.8, 1.5]), 0.6), (np.array([1.0, 3.0, 2.2]), 0.35))
MARGIN = 0.1


def room_lattice(res):
    """(field fp32 [res]^3, spacing, origin): positive in the room's solid parts (outside the walls, inside the table and the
    spheres), the zero level on their surfaces"""
    axes = [np.linspace(ROOM_LO[d] - MARGIN, ROOM_HI[d] + MARGIN, res) for d in range(3)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    P = (X, Y, Z)
    inner = np.min([np.minimum(P[d] - ROOM_LO[d], ROOM_HI[d] - P[d]) for d in range(3)], axis=0)
    f = -inner
    table = np.min([TABLE_H[d] - np.abs(P[d] - TABLE_C[d]) for d in range(3)], axis=0)
    f = np.maximum(f, table)
    for c, r in SPHERES:
        f = np.maximum(f, r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2))
    return f.astype(np.float32), [a[1] - a[0] for a in axes], [a[0] for a in axes]


def _box_faces(c, h):
    """(origin, edge u, edge v, area) of the six faces of the box centre c, half extents h"""
    out = []
    for d in range(3):
        e1, e2 = (d + 1) % 3, (d + 2) % 3
        for s in (-1, 1):
            o = c.astype(np.float64).copy()
            o[d] += s * h[d]
            o[e1] -= h[e1]
            o[e2] -= h[e2]
            u, v = np.zeros(3), np.zeros(3)
            u[e1], v[e2] = 2 * h[e1], 2 * h[e2]
            out.append((o, u, v, 4 * h[e1] * h[e2]))
    return out


def room_surface_points(n, seed=0):
    """n points drawn uniformly (by area) on the room's exact surface"""
    rng = np.random.default_rng(seed)
    faces = _box_faces((ROOM_LO + ROOM_HI) / 2, (ROOM_HI - ROOM_LO) / 2) + _box_faces(TABLE_C, TABLE_H)
    parts = [(f, f[3]) for f in faces] + [(s, 4 * np.pi * s[1] ** 2) for s in SPHERES]
    w = np.array([a for _, a in parts])
    pick = rng.choice(len(parts), size=n, p=w / w.sum())
    pts = np.empty((n, 3))
    for k, (p, _) in enumerate(parts):
        m = pick == k
        cnt = int(m.sum())
        if len(p) == 4:
            a, b = rng.uniform(size=(cnt, 1)), rng.uniform(size=(cnt, 1))
            pts[m] = p[0] + a * p[1] + b * p[2]
        else:
            g = rng.normal(size=(cnt, 3))
            pts[m] = p[0] + p[1] * g / np.linalg.norm(g, axis=1, keepdims=True)
    return pts


def bumpy_lattice(res=96):
    """a closed, asymmetric object about 0.7 m across (three blobs: no rotational symmetry, so ICP has one answer)"""
    ax = np.linspace(-0.5, 0.5, res)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")

    def blob(c, r):
        return 1.0 - np.sqrt(((X - c[0]) / r[0]) ** 2 + ((Y - c[1]) / r[1]) ** 2 + ((Z - c[2]) / r[2]) ** 2)

    f = np.maximum(np.maximum(blob((0, 0, 0), (0.25, 0.18, 0.12)), blob((0.25, 0.1, 0.05), (0.1, 0.1, 0.1))),
                   blob((-0.15, -0.1, 0.1), (0.05, 0.06, 0.2)))
    return f.astype(np.float32), [ax[1] - ax[0]] * 3, [ax[0]] * 3


def rigid(axis, deg, t):
    """4x4 rotation by deg about axis, then translation t"""
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    M[:3, 3] = t
    return M
