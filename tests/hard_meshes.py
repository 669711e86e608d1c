"""Small deterministic meshes built to break assembly (plain numpy: importable without a GPU).

Every function returns ``(points (nv, d) float64, cells (nc, d + 1) int64)``; none has more than a few hundred cells.
What each one reaches:

``fan(k, rx, ry)``     k triangles around the origin: the centre row has k + 1 (P1), 3 k + 1 (P2), 6 k + 1 (P3) entries
``spindle(k)``         k tetrahedra around one pole-pole edge: the pole rows have k + 2 (P1), 4 k + 3 (P2), 10 k + 4 (P3)
``stretched(d)``       a lattice scaled by (1e4, 1) / (1, 1e-2, 1e-4) and sheared by 0.37: entries spanning >= 1e5
``squashed()``         a 3-D lattice with z * 1e-6: nearly flat tetrahedra with O(1) edges
``tiny_far(d)``        a lattice * 1e-3 moved to +1e3 on every axis: millimetre cells far from the origin
``flipped(mesh)``      any of them with two vertices swapped in every second cell: det J of both signs

The storage width of a row is its length rounded up to ``OX_KV`` = 2; set-up refuses a width of 256.  ``FAN_K`` /
``SPINDLE_K`` list, per element degree, the k whose widest row lands just below and just above every point at which the
row kernels change their launch (ox_assemble.hip, launch_rows_t: 4 -> 2 waves per block above 70 entries, 2 -> 1 above 140;
67 and 134 with a per-cell viscosity, and in launch_scalar_cellvisc_t, which sizes the launches of ox_scalar_rows_cellvisc and
ox_scalar_rows_supg by the same rule) and at the last width the position bytes hold (254)."""
from __future__ import annotations

import numpy as np

from oracle import ipcs_oracle as O

KV = 2  # OX_KV


def fan(k: int, rx: float = 1.0, ry: float = 1.0):
    assert k >= 3
    th = 2.0 * np.pi * np.arange(k) / k
    pts = np.concatenate([np.zeros((1, 2)), np.stack([rx * np.cos(th), ry * np.sin(th)], axis=1)])
    i = np.arange(k)
    cells = np.stack([np.zeros(k, dtype=np.int64), 1 + i, 1 + (i + 1) % k], axis=1).astype(np.int64)
    return pts, cells


def spindle(k: int, r: float = 1.0, h: float = 1.0):
    assert k >= 3
    th = 2.0 * np.pi * np.arange(k) / k
    pts = np.concatenate([[[0.0, 0.0, -h], [0.0, 0.0, h]], np.stack([r * np.cos(th), r * np.sin(th), np.zeros(k)], axis=1)])
    i = np.arange(k)
    cells = np.stack([np.zeros(k, dtype=np.int64), np.ones(k, dtype=np.int64), 2 + i, 2 + (i + 1) % k], axis=1).astype(np.int64)
    return pts, cells


def lattice(d: int, n: int | None = None):
    """The box / rectangle lattice of [-1, 1]^d (n = 6 per side in 2-D: 72 triangles; 3 in 3-D: 162 tetrahedra)."""
    if d == 2:
        n = 6 if n is None else n
        return O.create_rectangle_mesh([-1.0, -1.0], [1.0, 1.0], [n, n])
    n = 3 if n is None else n
    return O.create_box_mesh([-1.0] * 3, [1.0] * 3, [n, n, n])


def stretched(d: int):
    pts, cells = lattice(d)
    pts = pts * (np.array([1e4, 1.0]) if d == 2 else np.array([1.0, 1e-2, 1e-4]))
    pts[:, 0] += 0.37 * pts[:, 1]
    if d == 3:
        pts[:, 1] += 0.37 * pts[:, 2]
    return pts, cells


def squashed():
    pts, cells = lattice(3)
    return pts * np.array([1.0, 1.0, 1e-6]), cells


def tiny_far(d: int):
    pts, cells = lattice(d)
    return pts * 1e-3 + 1e3, cells


def flipped(mesh):
    """Two vertices swapped in every second cell -- cells 1 and 2 of each four: a lattice of triangles already alternates
    its orientation cell by cell, so flipping cells 1, 3, 5, ... would only make it uniform."""
    pts, cells = mesh
    cells = cells.copy()
    sel = flipped_cells(cells.shape[0])
    cells[sel] = cells[sel][:, [1, 0] + list(range(2, cells.shape[1]))]
    return pts, cells


def flipped_cells(nc: int) -> np.ndarray:
    return np.nonzero(np.isin(np.arange(nc) % 4, (1, 2)))[0]


def signed_det(mesh) -> np.ndarray:
    pts, cells = mesh
    d = pts.shape[1]
    J = np.stack([pts[cells[:, a]] - pts[cells[:, 0]] for a in range(1, d + 1)], axis=2)
    return np.linalg.det(J)


def aspect_ratio(mesh) -> np.ndarray:
    """Longest edge over shortest height of every cell (1 / (|grad lambda_a| max) is the shortest height)."""
    pts, cells = mesh
    d = pts.shape[1]
    G, _ = O.cell_geometry(pts, cells)
    hmin = 1.0 / np.linalg.norm(G, axis=2).max(axis=1)
    x = pts[cells]
    emax = np.zeros(cells.shape[0])
    for a in range(d + 1):
        for b in range(a):
            emax = np.maximum(emax, np.linalg.norm(x[:, a] - x[:, b], axis=1))
    return emax / hmin


def fan_row(k: int, degree: int) -> int:
    return {1: k + 1, 2: 3 * k + 1, 3: 6 * k + 1}[degree]


def spindle_row(k: int, degree: int) -> int:
    return {1: k + 2, 2: 4 * k + 3, 3: 10 * k + 4}[degree]


def width_of(row_len: int) -> int:
    return max(KV, (row_len + KV - 1) // KV * KV)


def widest_row(mesh, degree: int) -> int:
    """Longest row of the Lagrange space of ``degree`` on the mesh, counted from the oracle's dof map (no device)."""
    pts, cells = mesh
    cd, n, _ = O.build_dofmap(cells, pts.shape[0], degree)
    nd = cd.shape[1]
    keys = np.unique((np.repeat(cd, nd, axis=1).ravel() * np.int64(n) + np.tile(cd, (1, nd)).ravel()))
    return int(np.bincount(keys // n, minlength=n).max())


# k per degree: (k, designed storage width of the widest row).  Each pair of neighbours straddles one switch point of
# launch_rows_t (width <= 70 | > 70, <= 140 | > 140; with nut <= 67 | > 67, <= 134 | > 134); the last is the widest row
# set-up accepts.  The widths are the nearest ones the element reaches.
FAN_K = {
    1: [(65, 66), (67, 68), (69, 70), (71, 72), (133, 134), (135, 136), (139, 140), (141, 142), (253, 254)],
    2: [(21, 64), (22, 68), (23, 70), (24, 74), (44, 134), (45, 136), (46, 140), (47, 142), (84, 254)],
    3: [(10, 62), (11, 68), (12, 74), (22, 134), (23, 140), (24, 146), (42, 254)],
}
SPINDLE_K = {
    1: [(64, 66), (66, 68), (68, 70), (70, 72), (132, 134), (134, 136), (138, 140), (140, 142), (252, 254)],
    2: [(15, 64), (16, 68), (17, 72), (32, 132), (33, 136), (34, 140), (35, 144), (62, 252)],
    3: [(6, 64), (7, 74), (13, 134), (14, 144), (25, 254)],
}
WIDEST = {("fan", 1): 253, ("fan", 2): 84, ("fan", 3): 42, ("spindle", 1): 252, ("spindle", 2): 62, ("spindle", 3): 25}


def widest(kind: str, degree: int):
    k = WIDEST[(kind, degree)]
    return fan(k, 3.0, 1.0) if kind == "fan" else spindle(k)


def zoo(d: int, degree: int):
    """name -> mesh for a velocity space of ``degree``: the widest fan / spindle of that element, the stretched, squashed,
    far-away and negatively oriented meshes.  (P3 on tetrahedra: the spindle and the stretched lattice only.)"""
    if d == 2:
        return {"fan254": widest("fan", degree), "stretched": stretched(2), "tiny_far": tiny_far(2),
                "flipped": flipped(stretched(2))}
    out = {"spindle254": widest("spindle", degree), "stretched": stretched(3)}
    if degree < 3:
        out.update({"squashed": squashed(), "tiny_far": tiny_far(3), "flipped": flipped(stretched(3))})
    return out
