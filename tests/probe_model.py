"""Numpy model of point location and evaluation (what csrc/ox_probe.hip computes, by brute force).

Location: EVERY cell is tested; a point is in a cell when all barycentric coordinates are >= -tol, and the answer is the
LOWEST such cell id (-1: none) -- the rule of ``oasisx_amd.geometry``.  Evaluation: ``fem.lagrange_basis`` on the
space's ``cell_dofs`` in kernel cell order.  The partition rule: locate among the rank's window cells, owner = the owner
of the first vertex of the lowest containing cell."""
from __future__ import annotations

import numpy as np


def barycentric(coords, cells, cell_ids, x):
    """(len(cell_ids), npts, d + 1): barycentric coordinates of every point in every listed cell."""
    xc = coords[cells[cell_ids]]  # (m, d+1, d)
    d = coords.shape[1]
    J = np.moveaxis(xc[:, 1:, :] - xc[:, :1, :], 1, 2)  # columns = edge vectors
    Jinv = np.linalg.inv(J)  # rows = grad(lambda_1..d)
    r = x[None, :, :] - xc[:, None, 0, :]  # (m, n, d)
    lam = np.einsum("mak,mnk->mna", Jinv, r)
    return np.concatenate([1.0 - lam.sum(axis=2, keepdims=True), lam], axis=2)


def locate(coords, cells, x, tol=1e-10, cell_ids=None, chunk=256):
    """(cell, bary): per point the lowest id among ``cell_ids`` (default: all cells) that contains it, -1 if none, and
    its barycentric coordinates there (NaN if none)."""
    coords, cells = np.asarray(coords, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)[:, : coords.shape[1]]
    ids = np.arange(cells.shape[0]) if cell_ids is None else np.sort(np.asarray(cell_ids, dtype=np.int64))
    n, d = x.shape
    out = np.full(n, -1, dtype=np.int64)
    bary = np.full((n, d + 1), np.nan)
    for p0 in range(0, n, chunk):
        lam = barycentric(coords, cells, ids, x[p0:p0 + chunk])  # (m, k, d+1)
        inside = lam.min(axis=2) >= -tol  # (m, k)
        hit = inside.any(axis=0)
        first = np.argmax(inside, axis=0)  # ids ascending: the first hit is the lowest id
        k = np.arange(first.shape[0])
        out[p0:p0 + chunk] = np.where(hit, ids[first], -1)
        bary[p0:p0 + chunk] = np.where(hit[:, None], lam[first, k], np.nan)
    return out, bary


def evaluate(V, u, x, cell, bary=None):
    """Values (n, k) at the points ``x`` lying in the mesh cells ``cell`` of the field with dof array ``u`` (n_local,) or
    (n_local, k) on the scalar space ``V``; NaN rows for cell -1."""
    from oasisx_amd import fem

    mesh = V.mesh
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    u = np.asarray(u, dtype=np.float64)
    u = u[:, None] if u.ndim == 1 else u
    cell = np.asarray(cell, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)[:, : mesh.gdim]
    out = np.full((x.shape[0], u.shape[1]), np.nan)
    ok = np.nonzero(cell >= 0)[0]
    if ok.size == 0:
        return out
    kpos = V.kernel_cell_index(cell[ok])
    assert (kpos >= 0).all(), "the model was asked for a cell the space does not hold"
    if bary is None:
        lam = np.stack([barycentric(coords, cells, cell[i:i + 1], x[i:i + 1])[0, 0] for i in ok])
    else:
        lam = np.asarray(bary)[ok]
    phi = fem.lagrange_basis(mesh.gdim, V.degree, lam)  # (n, nd)
    cd = V.cell_dofs.cpu().numpy()[kpos]  # (n, nd)
    out[ok] = np.einsum("na,nak->nk", phi, u[cd])
    return out


def owners(mesh, parts, x, tol=1e-10):
    """The partition rule on every rank: list of (rank, mask of the points the rank keeps, its cells c*)."""
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    out = []
    for part in parts:
        c, _ = locate(coords, cells, x, tol, cell_ids=part.win_cells.cpu().numpy())
        vown = part.vown.cpu().numpy()
        mine = (c >= 0) & (vown[cells[np.maximum(c, 0), 0]] == part.rank)
        out.append((part.rank, mine, c))
    return out


def sample_points(mesh, n_random, n_vertices, n_edges, seed=0, n_centroids=0, n_faces=0):
    """Test points inside the mesh: random convex combinations of the vertices of random cells (strictly interior),
    vertices, edge midpoints, cell centroids and (3-D) face centroids."""
    rng = np.random.default_rng(seed)
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    d = coords.shape[1]
    pts = []
    c = rng.integers(0, cells.shape[0], n_random)
    w = rng.dirichlet(np.ones(d + 1) * 2.0, n_random)
    w = 0.02 + (1.0 - 0.02 * (d + 1)) * w  # every lambda >= 0.02: four orders above the tolerance, and more
    pts.append(np.einsum("na,nak->nk", w, coords[cells[c]]))
    pts.append(coords[rng.integers(0, coords.shape[0], n_vertices)])
    c = rng.integers(0, cells.shape[0], n_edges)
    a = rng.integers(0, d + 1, n_edges)
    b = (a + 1 + rng.integers(0, d, n_edges)) % (d + 1)
    pts.append(0.5 * (coords[cells[c, a]] + coords[cells[c, b]]))
    if n_centroids:
        c = rng.integers(0, cells.shape[0], n_centroids)
        pts.append(coords[cells[c]].mean(axis=1))
    if n_faces and d == 3:
        c = rng.integers(0, cells.shape[0], n_faces)
        skip = rng.integers(0, 4, n_faces)
        keep = np.stack([np.delete(np.arange(4), s) for s in skip])
        pts.append(coords[cells[c[:, None], keep]].mean(axis=1))
    return np.concatenate(pts, axis=0)
