"""Simplicial meshes with the small DOLFINx-shaped surface the oasisx callers touch
(reference demo/taylor_green.py:126-139, test/test_tentative_velocity.py:90-128,
bcs.py:99-100,245-250): generators, facet/edge tables, ``meshtags``, entity location.

Mesh arrays live as torch tensors on the setup device (the GPU when there is one) so
that 128^3 x 6 tetrahedra are generated and indexed there; numpy views are made on
demand for the host-side callers.
"""
from __future__ import annotations

import enum
import itertools

import numpy as np
import torch


def default_device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device("cpu")


class CellType(enum.Enum):
    triangle = 2
    tetrahedron = 3


class _Comm:
    """Stand-in for the MPI communicator attribute callers pass around; the data path
    uses RCCL (see oasisx_amd.parallel), not MPI."""

    def __init__(self, rank=0, size=1):
        self.rank, self.size = rank, size

    def allreduce(self, v, op=None):
        return v

    def Barrier(self):
        pass


COMM_WORLD = _Comm()


class _UflCell:
    def __init__(self, name):
        self.cellname = name


class _IndexMap:
    def __init__(self, n):
        self.size_local = int(n)
        self.num_ghosts = 0
        self.size_global = int(n)


class Geometry:
    def __init__(self, mesh):
        self._mesh = mesh
        self.dim = mesh.gdim

    @property
    def x(self) -> np.ndarray:
        """(n_vertices, 3) vertex coordinates (zero padded), as in DOLFINx."""
        m = self._mesh
        if m._x3 is None:
            x = np.zeros((m.num_vertices, 3))
            x[:, : m.gdim] = m.coords.cpu().numpy()
            m._x3 = x
        return m._x3


class Topology:
    def __init__(self, mesh):
        self._mesh = mesh
        self.dim = mesh.gdim

    def create_connectivity(self, d0, d1):
        self._mesh._entities(d0)
        self._mesh._entities(d1)

    def create_entities(self, dim):
        self._mesh._entities(dim)

    def index_map(self, dim):
        m = self._mesh
        if dim == m.gdim:
            return _IndexMap(m.num_cells)
        if dim == 0:
            return _IndexMap(m.num_vertices)
        return _IndexMap(m._entities(dim)[0].shape[0])

    def cell_name(self):
        return self._mesh.cellname

    @property
    def _cpp_object(self):
        return self


class Mesh:
    """coords: (nv, gdim) float64, cells: (nc, gdim+1) int64 vertex ids."""

    def __init__(self, coords: torch.Tensor, cells: torch.Tensor, comm=COMM_WORLD):
        self.coords = coords.to(torch.float64).contiguous()
        self.cells = cells.to(torch.int64).contiguous()
        self.device = self.coords.device
        self.gdim = int(coords.shape[1])
        assert cells.shape[1] == self.gdim + 1, "simplicial cells only"
        self.num_vertices = int(coords.shape[0])
        self.num_cells = int(cells.shape[0])
        self.cellname = "triangle" if self.gdim == 2 else "tetrahedron"
        self.comm = comm
        self._x3 = None
        self._ent = {}
        self._tcells = None
        self.periodic = None  # a PeriodicMap on meshes made by make_periodic
        self.geometry = Geometry(self)
        self.topology = Topology(self)

    def ufl_cell(self):
        return _UflCell(self.cellname)

    # ---- entity tables (host, lazy; not used on the hot path) -------------------------
    def _entities(self, dim):
        """(entity_vertices (ne, dim+1) sorted rows, cell_entities (nc, nloc))."""
        if dim in self._ent:
            return self._ent[dim]
        cells = self.cells.cpu().numpy()
        nvl = self.gdim + 1
        if dim == self.gdim:
            res = (np.sort(cells, axis=1), np.arange(self.num_cells)[:, None])
        elif dim == 0:
            res = (np.arange(self.num_vertices)[:, None], cells)
        else:
            combos = list(itertools.combinations(range(nvl), dim + 1))
            sub = np.stack([np.sort(cells[:, list(c)], axis=1) for c in combos], axis=1)
            flat = sub.reshape(-1, dim + 1)
            key = np.zeros(flat.shape[0], dtype=np.int64)
            for k in range(dim + 1):
                key = key * np.int64(self.num_vertices) + flat[:, k]
            uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
            res = (flat[first], inv.reshape(self.num_cells, len(combos)))
        self._ent[dim] = res
        return res

    def exterior_facets(self) -> np.ndarray:
        """Facets of one cell, without the facets a periodic mesh identifies (``periodic_facets``)."""
        _, cf = self._entities(self.gdim - 1)
        counts = np.bincount(cf.ravel())
        ext = np.nonzero(counts == 1)[0].astype(np.int32)
        if self.periodic is not None:
            ext = np.setdiff1d(ext, self.periodic.facets).astype(np.int32)
        return ext

    def periodic_facets(self) -> np.ndarray:
        """Facets on the identified faces of a periodic mesh (both images), ascending; empty on any other mesh."""
        if self.periodic is None:
            return np.zeros(0, dtype=np.int32)
        return self.periodic.facets

    def topological_cells(self) -> torch.Tensor:
        """Cell -> vertex CLASS ids (0 .. n_free_vertices - 1) of a periodic mesh: the table dofs are numbered from.
        ``cells`` itself on any other mesh."""
        if self.periodic is None:
            return self.cells
        if self._tcells is None:
            vt = torch.from_numpy(self.periodic.vertex_topo).to(self.device)
            self._tcells = vt[self.cells].contiguous()
        return self._tcells

    def h(self, dim, entities) -> np.ndarray:
        """Largest vertex distance of each cell (dolfinx.mesh.Mesh.h for cells)."""
        assert dim == self.gdim
        x = self.coords.cpu().numpy()
        c = self.cells.cpu().numpy()[np.asarray(entities)]
        hmax = np.zeros(c.shape[0])
        for a, b in itertools.combinations(range(self.gdim + 1), 2):
            hmax = np.maximum(hmax, np.linalg.norm(x[c[:, a]] - x[c[:, b]], axis=1))
        return hmax


# ---- arbitrary simplicial meshes ---------------------------------------------------------------


def from_arrays(coords, cells, comm=None, device=None) -> Mesh:
    """Mesh from vertex coordinates (nv, gdim) and cell->vertex ids (nc, gdim+1): any conforming
    triangle / tetrahedron mesh, in any cell order and vertex orientation (the stand-in for the
    reference's stubbed ``import_mesh``, src/oasisx/mesh.py:13-15).  Locality of the kernel data is
    recovered by the spatial ordering of dofs and cells, not assumed from the input."""
    dev = default_device() if device is None else torch.device(device)
    c = torch.as_tensor(np.asarray(coords, dtype=np.float64)).to(dev)
    t = torch.as_tensor(np.asarray(cells, dtype=np.int64)).to(dev)
    return Mesh(c, t, comm if comm is not None else COMM_WORLD)


# ---- mesh files -----------------------------------------------------------------------------------


def _read_medit(path):
    """Medit ASCII ``.mesh``: ``Vertices`` (x y [z] ref), ``Triangles`` / ``Tetrahedra`` (1-based, ref)."""
    tok = open(path).read().split()
    i, dim, pts, tri, tet = 0, 3, None, None, None

    def block(n, width):
        nonlocal i
        a = np.asarray(tok[i:i + n * width], dtype=np.float64).reshape(n, width)
        i += n * width
        return a

    while i < len(tok):
        w = tok[i].lower()
        i += 1
        if w == "dimension":
            dim = int(tok[i])
            i += 1
        elif w == "vertices":
            n = int(tok[i])
            i += 1
            pts = block(n, dim + 1)[:, :dim]
        elif w == "triangles":
            n = int(tok[i])
            i += 1
            tri = block(n, 4)[:, :3].astype(np.int64) - 1
        elif w == "tetrahedra":
            n = int(tok[i])
            i += 1
            tet = block(n, 5)[:, :4].astype(np.int64) - 1
        elif w == "end":
            break
    if pts is None:
        raise ValueError(f"{path}: no Vertices section")
    cells = tet if tet is not None and len(tet) else tri
    if cells is None:
        raise ValueError(f"{path}: neither Tetrahedra nor Triangles")
    if cells.shape[1] == 3 and pts.shape[1] == 3 and np.ptp(pts[:, 2]) == 0.0:
        pts = pts[:, :2]  # a planar triangle mesh written with z = const
    return pts, cells


def _read_plain(path):
    """Plain text: ``vertices <n> <gdim>`` + n coordinate lines, ``cells <m> <k>`` + m lines of k 0-based vertex ids
    (``#`` starts a comment)."""
    lines = [ln.split("#", 1)[0].split() for ln in open(path)]
    lines = [ln for ln in lines if ln]
    i, pts, cells = 0, None, None
    while i < len(lines):
        head = lines[i]
        if head[0].lower() == "vertices":
            n, d = int(head[1]), int(head[2])
            pts = np.asarray(lines[i + 1:i + 1 + n], dtype=np.float64).reshape(n, d)
            i += 1 + n
        elif head[0].lower() == "cells":
            m, k = int(head[1]), int(head[2])
            cells = np.asarray(lines[i + 1:i + 1 + m], dtype=np.int64).reshape(m, k)
            i += 1 + m
        else:
            raise ValueError(f"{path}: unexpected line {' '.join(head)!r}")
    if pts is None or cells is None:
        raise ValueError(f"{path}: needs a 'vertices' and a 'cells' section")
    return pts, cells


# Gmsh element types of the simplices: number of nodes
_GMSH_NODES = {15: 1, 1: 2, 2: 3, 4: 4}


def _read_gmsh(path):
    """Gmsh ``.msh`` ASCII, format 2.2 or 4.1 (what ``gmsh -format msh2 / msh4`` writes and
    ``dolfinx.io.gmshio.read_from_msh`` reads for the reference's users): first-order points, lines, triangles and
    tetrahedra.  Returns (points (n, 3), {element type: (node ids 0-based (m, k), physical tag (m,))})."""
    lines = open(path).read().split("\n")
    sec, i = {}, 0
    while i < len(lines):
        ln = lines[i].strip()
        if ln.startswith("$") and not ln.startswith("$End"):
            j = i + 1
            while j < len(lines) and lines[j].strip() != "$End" + ln[1:]:
                j += 1
            sec[ln[1:]] = lines[i + 1:j]
            i = j
        i += 1
    if "MeshFormat" not in sec:
        raise ValueError(f"{path}: not a Gmsh .msh file")
    fmt = sec["MeshFormat"][0].split()
    version, binary = float(fmt[0]), int(fmt[1])
    if binary:
        raise ValueError(f"{path}: binary .msh files are not read (write ASCII: gmsh -format msh4 / Mesh.Binary = 0)")
    elems = {}

    def add(etype, nodes, tag):
        if etype in _GMSH_NODES:
            elems.setdefault(etype, ([], []))
            elems[etype][0].append(nodes)
            elems[etype][1].append(tag)

    if version < 3.0:
        body = sec["Nodes"]
        n = int(body[0])
        tab = np.asarray([ln.split() for ln in body[1:1 + n]], dtype=np.float64)
        ids, pts = tab[:, 0].astype(np.int64), tab[:, 1:4]
        body = sec["Elements"]
        for ln in body[1:1 + int(body[0])]:
            t = [int(v) for v in ln.split()]
            etype, ntags = t[1], t[2]
            add(etype, t[3 + ntags:3 + ntags + _GMSH_NODES.get(etype, 0)], t[3] if ntags > 0 else 0)
    else:
        phys = {}  # (entity dim, entity tag) -> first physical tag
        if "Entities" in sec:
            body = sec["Entities"]
            counts = [int(v) for v in body[0].split()]
            k = 1
            for dim, cnt in enumerate(counts):
                for _ in range(cnt):
                    t = body[k].split()
                    k += 1
                    off = 4 if dim == 0 else 7  # tag + a point, or tag + a bounding box
                    nph = int(t[off])
                    # (Gmsh 4.1 writes the physical tag of an entity with REVERSED orientation negative: the group is |tag|)
                    phys[(dim, int(t[0]))] = abs(int(t[off + 1])) if nph > 0 else 0
        body = sec["Nodes"]
        nblocks = int(body[0].split()[0])
        k, ids, pts = 1, [], []
        for _ in range(nblocks):
            h = [int(v) for v in body[k].split()]
            nn = h[3]
            ids += [int(v) for v in body[k + 1:k + 1 + nn]]
            pts += [[float(v) for v in ln.split()[:3]] for ln in body[k + 1 + nn:k + 1 + 2 * nn]]
            k += 1 + 2 * nn
        ids, pts = np.asarray(ids, dtype=np.int64), np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        body = sec["Elements"]
        nblocks = int(body[0].split()[0])
        k = 1
        for _ in range(nblocks):
            edim, etag, etype, ne = (int(v) for v in body[k].split())
            tag = phys.get((edim, etag), 0)
            for ln in body[k + 1:k + 1 + ne]:
                add(etype, [int(v) for v in ln.split()[1:1 + _GMSH_NODES.get(etype, 0)]], tag)
            k += 1 + ne
    lookup = np.full(int(ids.max()) + 1, -1, dtype=np.int64)
    lookup[ids] = np.arange(ids.shape[0])
    out = {}
    for etype, (nodes, tags) in elems.items():
        out[etype] = (lookup[np.asarray(nodes, dtype=np.int64)], np.asarray(tags, dtype=np.int32))
    return pts, out


def read_gmsh(filename: str, comm=None, device=None, gdim: int | None = None):
    """``dolfinx.io.gmshio.read_from_msh`` for first-order simplicial meshes: (mesh, cell_tags, facet_tags) from a Gmsh
    ASCII ``.msh`` file (2.2 or 4.1).  The tags are the physical groups of the cells and of the facet elements (lines
    in 2-D, triangles in 3-D) the file lists -- ``MeshTags`` ready for ``DirichletBC(..., LocatorMethod.TOPOLOGICAL,
    (facet_tags, id))`` and ``PressureBC(value, (facet_tags, id))``.  ``gdim``: 2 drops the z coordinate (default: 2
    when the file holds no tetrahedron and z is constant)."""
    pts, el = _read_gmsh(filename)
    if gdim is None:
        gdim = 3 if 4 in el else (2 if np.ptp(pts[:, 2]) == 0.0 else 3)
    ctype, ftype = (4, 2) if gdim == 3 and 4 in el else (2, 1)
    if ctype not in el:
        raise ValueError(f"{filename}: no {'tetrahedra' if ctype == 4 else 'triangles'} found")
    cells, ctag = el[ctype]
    used = np.zeros(pts.shape[0], dtype=bool)
    used[cells.ravel()] = True
    new = np.cumsum(used) - 1
    mesh = from_arrays(pts[used][:, :gdim], new[cells], comm=comm, device=device)
    cell_tags = MeshTags(mesh, gdim, np.arange(cells.shape[0], dtype=np.int32), ctag)
    fidx, fval = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if ftype in el:
        fn, ft = el[ftype]
        keep = used[fn].all(axis=1)
        fn, ft = np.sort(new[fn[keep]], axis=1), ft[keep]
        ev, _ = mesh._entities(gdim - 1)  # facet -> sorted vertices
        nv = mesh.num_vertices

        def key(a):
            k = np.zeros(a.shape[0], dtype=np.int64)
            for c in range(a.shape[1]):
                k = k * np.int64(nv) + a[:, c]
            return k
        ka, kf = key(ev), key(fn)
        order = np.argsort(ka)
        pos = np.searchsorted(ka[order], kf)
        ok = (pos < ka.shape[0]) & (ka[order][np.minimum(pos, ka.shape[0] - 1)] == kf)
        idx = order[pos[ok]]
        srt = np.argsort(idx)
        fidx, fval = idx[srt].astype(np.int32), ft[ok][srt]
        first = np.ones(fidx.shape[0], dtype=bool)
        first[1:] = fidx[1:] != fidx[:-1]
        fidx, fval = fidx[first], fval[first]
    return mesh, cell_tags, MeshTags(mesh, gdim - 1, fidx, fval)


def read_mesh(filename: str, comm=None, device=None) -> Mesh:
    """Simplicial mesh from a file: ``.npz`` (arrays ``points``/``coords`` and ``cells``), Medit ASCII ``.mesh``,
    Gmsh ASCII ``.msh`` (2.2 / 4.1; with its physical groups: :func:`read_gmsh`) or the plain text format of
    :func:`write_mesh`.  Cells may come in any order and orientation; unused
    vertices are dropped.  No gmsh / XDMF / ADIOS2 dependency."""
    ext = filename.rsplit(".", 1)[-1].lower()
    if ext == "npz":
        z = np.load(filename)
        pts = np.asarray(z["points"] if "points" in z.files else z["coords"], dtype=np.float64)
        cells = np.asarray(z["cells"], dtype=np.int64)
    elif ext == "mesh":
        pts, cells = _read_medit(filename)
    elif ext == "msh":  # Gmsh ASCII 2.2 / 4.1 (the physical groups: read_gmsh)
        return read_gmsh(filename, comm=comm, device=device)[0]
    else:
        pts, cells = _read_plain(filename)
    if cells.ndim != 2 or cells.shape[1] != pts.shape[1] + 1:
        raise ValueError(f"{filename}: {cells.shape[1]}-vertex cells in {pts.shape[1]}-D: triangles in 2-D or tetrahedra in 3-D")
    if cells.min() < 0 or cells.max() >= pts.shape[0]:
        raise ValueError(f"{filename}: cell vertex index out of range")
    used = np.zeros(pts.shape[0], dtype=bool)
    used[cells.ravel()] = True
    if not used.all():
        new = np.cumsum(used) - 1
        pts, cells = pts[used], new[cells]
    return from_arrays(pts, cells, comm=comm, device=device)


def write_mesh(mesh: Mesh, filename: str):
    """Write ``mesh`` as ``.npz`` (points, cells) or as plain text (see :func:`read_mesh`)."""
    pts, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    if filename.lower().endswith(".npz"):
        np.savez(filename, points=pts, cells=cells)
        return
    with open(filename, "w") as f:
        f.write(f"# oasisx_amd mesh\nvertices {pts.shape[0]} {pts.shape[1]}\n")
        np.savetxt(f, pts, fmt="%.17g")
        f.write(f"cells {cells.shape[0]} {cells.shape[1]}\n")
        np.savetxt(f, cells, fmt="%d")


def import_mesh(filename: str) -> Mesh:
    """The reference's ``oasisx.import_mesh`` (src/oasisx/mesh.py:13-15 -- a stub there that prints
    the file name and returns a unit square): here it reads the file."""
    return read_mesh(filename)


# ---- generators (DOLFINx layouts) --------------------------------------------------------


def create_rectangle(comm, points, n, cell_type=CellType.triangle, device=None, **kwargs) -> Mesh:
    """dolfinx.mesh.create_rectangle, triangles, DiagonalType.right: each quad
    (v0 v1 / v2 v3) is cut into [v0, v1, v3] and [v0, v2, v3]."""
    assert cell_type == CellType.triangle
    dev = default_device() if device is None else torch.device(device)
    nx, ny = int(n[0]), int(n[1])
    p0, p1 = points
    xs = torch.linspace(float(p0[0]), float(p1[0]), nx + 1, dtype=torch.float64, device=dev)
    ys = torch.linspace(float(p0[1]), float(p1[1]), ny + 1, dtype=torch.float64, device=dev)
    Y, X = torch.meshgrid(ys, xs, indexing="ij")
    coords = torch.stack([X.reshape(-1), Y.reshape(-1)], dim=1)
    iy, ix = torch.meshgrid(torch.arange(ny, device=dev), torch.arange(nx, device=dev), indexing="ij")
    v0 = (iy * (nx + 1) + ix).reshape(-1)
    v1, v2, v3 = v0 + 1, v0 + nx + 1, v0 + nx + 2
    cells = torch.stack([torch.stack([v0, v1, v3], 1), torch.stack([v0, v2, v3], 1)], dim=1)
    return Mesh(coords, cells.reshape(-1, 3), comm if comm is not None else COMM_WORLD)


def create_unit_square(comm, nx, ny, cell_type=CellType.triangle, device=None, **kwargs) -> Mesh:
    return create_rectangle(comm, [[0.0, 0.0], [1.0, 1.0]], [nx, ny], cell_type, device=device)


def create_box(comm, points, n, cell_type=CellType.tetrahedron, device=None, **kwargs) -> Mesh:
    """dolfinx.mesh.create_box, tetrahedra: every hexahedron is cut into the 6 tetrahedra
    that share its main diagonal v0-v7."""
    assert cell_type == CellType.tetrahedron
    dev = default_device() if device is None else torch.device(device)
    nx, ny, nz = (int(v) for v in n)
    p0, p1 = points
    ax = [torch.linspace(float(p0[k]), float(p1[k]), m + 1, dtype=torch.float64, device=dev)
          for k, m in enumerate((nx, ny, nz))]
    Z, Y, X = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    coords = torch.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], dim=1)
    iz, iy, ix = torch.meshgrid(torch.arange(nz, device=dev), torch.arange(ny, device=dev),
                                torch.arange(nx, device=dev), indexing="ij")
    sy, sz = nx + 1, (nx + 1) * (ny + 1)
    v0 = (iz * sz + iy * sy + ix).reshape(-1)
    v1, v2, v3 = v0 + 1, v0 + sy, v0 + 1 + sy
    v4, v5, v6, v7 = v0 + sz, v0 + sz + 1, v0 + sz + sy, v0 + sz + sy + 1
    tets = [(v0, v1, v3, v7), (v0, v1, v7, v5), (v0, v5, v7, v4),
            (v0, v3, v2, v7), (v0, v6, v4, v7), (v0, v2, v6, v7)]
    cells = torch.stack([torch.stack(t, 1) for t in tets], dim=1)
    return Mesh(coords, cells.reshape(-1, 4), comm if comm is not None else COMM_WORLD)


def refine_uniform(coords: np.ndarray, cells: np.ndarray):
    """One level of regular ("red") refinement of a simplicial mesh: every edge gets a midpoint vertex; a triangle
    becomes 4 triangles, a tetrahedron 4 corner tetrahedra plus its inner octahedron cut along its SHORTEST diagonal
    into 4 (Bey / Zhang: the cut that keeps the shape regularity).  Returns (coords, cells) with the old vertices
    first.  How large unstructured meshes are usually produced: a generator's mesh, refined uniformly."""
    coords = np.asarray(coords, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    nv, d = coords.shape
    le = [(0, 1), (0, 2), (1, 2)] if d == 2 else [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    a = np.stack([cells[:, i] for i, _ in le], axis=1)
    b = np.stack([cells[:, j] for _, j in le], axis=1)
    key = np.minimum(a, b) * np.int64(nv) + np.maximum(a, b)
    ukey, inv = np.unique(key.reshape(-1), return_inverse=True)
    mid = (nv + inv.reshape(key.shape)).astype(np.int64)  # midpoint vertex of each local edge
    new = 0.5 * (coords[ukey // nv] + coords[ukey % nv])
    X = np.concatenate([coords, new], axis=0)
    v = cells
    if d == 2:
        m01, m02, m12 = mid[:, 0], mid[:, 1], mid[:, 2]
        out = [np.stack(t, axis=1) for t in ((v[:, 0], m01, m02), (m01, v[:, 1], m12), (m02, m12, v[:, 2]), (m01, m12, m02))]
        return X, np.concatenate(out, axis=0)
    m01, m02, m03, m12, m13, m23 = (mid[:, k] for k in range(6))
    out = [np.stack(t, axis=1) for t in ((v[:, 0], m01, m02, m03), (m01, v[:, 1], m12, m13), (m02, m12, v[:, 2], m23),
                                          (m03, m13, m23, v[:, 3]))]
    # the octahedron m01 m02 m03 m12 m13 m23: its three diagonals join the midpoints of opposite edges
    diag = [(m01, m23, (m02, m03, m13, m12)), (m02, m13, (m01, m03, m23, m12)), (m03, m12, (m01, m02, m23, m13))]
    length = np.stack([np.linalg.norm(X[p_] - X[q_], axis=1) for p_, q_, _ in diag], axis=1)
    pick = np.argmin(length, axis=1)  # (ties: the first diagonal -- deterministic)
    octa = np.empty((cells.shape[0], 4, 4), dtype=np.int64)
    for k, (p_, q_, ring) in enumerate(diag):
        sel = pick == k
        for t in range(4):  # the 4 tetrahedra around the diagonal: (p, q, ring[t], ring[t+1])
            octa[sel, t] = np.stack([p_[sel], q_[sel], ring[t][sel], ring[(t + 1) % 4][sel]], axis=1)
    return X, np.concatenate(out + [octa.reshape(-1, 4)], axis=0)


def create_delaunay_box(comm, points, n, seed: int = 0, jitter: float = 0.35, device=None, refine: int = 0) -> Mesh:
    """A genuinely unstructured simplicial mesh of the box ``points = [p0, p1]``: Delaunay triangulation
    (scipy / Qhull) of a jittered (n+1)^dim lattice whose boundary points slide only inside their face /
    edge.  Vertex valence ranges from 1 to ~40 cells in 3-D -- nothing of a box mesh's topology is left.
    Flat cells on the hull are dropped and the total volume is checked.  The test and benchmark mesh for
    "what an unstructured mesh gets" (no reference counterpart: DOLFINx reads such meshes from files).
    ``refine`` > 0 refines the triangulation uniformly that many times (``refine_uniform``): Qhull takes minutes
    beyond ~3 x 10^5 points, a refined coarse Delaunay mesh reaches the BASELINE sizes in seconds and keeps the
    irregular valence of its coarse vertices."""
    import math

    from scipy.spatial import Delaunay

    p0, p1 = np.asarray(points[0], dtype=np.float64), np.asarray(points[1], dtype=np.float64)
    dim = p0.shape[0]
    rng = np.random.default_rng(seed)
    ax = np.linspace(-1.0, 1.0, n + 1)
    G = np.stack(np.meshgrid(*([ax] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    h = 2.0 / n
    move = (rng.random(G.shape) - 0.5) * 2.0 * jitter * h
    move[np.abs(G) > 1.0 - 1e-9] = 0.0  # a boundary point never leaves its face / edge / corner
    P = G + move
    T = Delaunay(P).simplices.astype(np.int64)
    x0 = P[T[:, 0]]
    J = np.stack([P[T[:, a]] - x0 for a in range(1, dim + 1)], axis=2)
    det = np.abs(np.linalg.det(J))
    keep = det > 1e-9 * h ** dim
    T = T[keep]
    assert abs(det[keep].sum() / math.factorial(dim) - 2.0 ** dim) < 1e-9
    X = p0 + (P + 1.0) * 0.5 * (p1 - p0)  # [-1, 1]^dim -> the box
    for _ in range(int(refine)):  # ``refine`` levels of uniform refinement: the Delaunay mesh at 8^refine times the cells
        X, T = refine_uniform(X, T)
    return from_arrays(X, T, comm=comm, device=device)


def create_unit_cube(comm, nx, ny, nz, cell_type=CellType.tetrahedron, device=None, **kwargs) -> Mesh:
    return create_box(comm, [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], [nx, ny, nz], cell_type, device=device)


# ---- periodic boundaries --------------------------------------------------------------------


class PeriodicMap:
    """Identification of the faces ``x_k = hi_k`` and ``x_k = lo_k`` of a mesh's bounding box, k in ``axes``.

    ``vertex_master`` (int64, all vertices, idempotent) names the image of a vertex that lies at ``lo`` on every
    periodic axis; ``vertex_topo`` numbers the classes 0 .. ``n_free_vertices`` - 1 in ascending master id;
    ``period`` holds the translation of every periodic axis (0 on the others); ``facets`` the identified facets."""

    def __init__(self, mesh, axes, lo, hi, period, atol, vertex_master, face_masks):
        self._mesh, self._face_masks, self._facets = mesh, face_masks, None
        self.axes = tuple(int(k) for k in axes)
        self.lo, self.hi, self.period, self.atol = lo, hi, period, atol
        self.vertex_master = vertex_master
        free = np.nonzero(vertex_master == np.arange(vertex_master.shape[0]))[0]
        self.n_free_vertices = int(free.shape[0])
        compact = np.full(vertex_master.shape[0], -1, dtype=np.int64)
        compact[free] = np.arange(free.shape[0])
        self.vertex_topo = compact[vertex_master]

    @property
    def facets(self) -> np.ndarray:
        """Ids (of ``mesh._entities(gdim - 1)``) of the facets on the identified faces, both images, ascending.  Found on
        first use: the facet table of a large mesh is built only for callers that name facets."""
        if self._facets is None:
            fv, _ = self._mesh._entities(self._mesh.gdim - 1)
            hit = np.zeros(fv.shape[0], dtype=bool)
            for on in self._face_masks:  # (all vertices on one face of the bounding box: a facet of one cell)
                hit |= on[fv].all(axis=1)
            self._facets = np.nonzero(hit)[0].astype(np.int32)
        return self._facets

    def is_periodic_facet(self, facets) -> np.ndarray:
        return np.isin(np.asarray(facets), self.facets)


def make_periodic(mesh: Mesh, axes, tol=None) -> Mesh:
    """``mesh`` with the face ``x_k = hi_k`` of its bounding box identified with ``x_k = lo_k`` for every k in ``axes``
    (translation by ``hi_k - lo_k``).  ``coords`` and ``cells`` stay the geometric mesh; the result carries
    ``mesh.periodic`` (:class:`PeriodicMap`), and function spaces on it number one dof per class of identified
    vertices, edges and faces.  ``tol``: matching tolerance relative to the span of each axis (default 1e-8).

    Raises ``ValueError`` naming the axis when the two faces do not carry matching vertices and matching facets, or
    when the mesh is fewer than three cells across the axis (two distinct edges would then join the same two vertex
    classes).  ``create_rectangle`` and ``create_box`` meshes match on every axis; a ``create_delaunay_box`` mesh
    jitters its face points independently, so its faces do not match and it is refused."""
    axes = tuple(sorted(set(int(k) for k in axes)))
    d = mesh.gdim
    if not axes or min(axes) < 0 or max(axes) >= d:
        raise ValueError(f"make_periodic: axes {axes} on a {d}-D mesh")
    if mesh.periodic is not None:
        raise ValueError("make_periodic: the mesh is periodic already")
    x = mesh.coords.cpu().numpy()
    cells = mesh.cells.cpu().numpy()
    nv = mesh.num_vertices
    lo, hi = x.min(axis=0), x.max(axis=0)
    span = hi - lo
    rtol = 1e-8 if tol is None else float(tol)
    atol = rtol * span
    vm = np.arange(nv, dtype=np.int64)
    period = np.zeros(d)
    masks = []
    others_of = {k: [j for j in range(d) if j != k] for k in axes}
    for k in axes:
        if not span[k] > 0.0:
            raise ValueError(f"make_periodic: axis {k}: the mesh has no extent")
        period[k] = span[k]
        on_lo, on_hi = np.abs(x[:, k] - lo[k]) <= atol[k], np.abs(x[:, k] - hi[k]) <= atol[k]
        il, ih = np.nonzero(on_lo)[0], np.nonzero(on_hi)[0]
        if il.shape[0] != ih.shape[0]:
            raise ValueError(f"make_periodic: axis {k}: {il.shape[0]} vertices on the lo face, {ih.shape[0]} on the hi face: "
                             "the vertices of the two faces do not match")
        oth = others_of[k]
        # pair every hi vertex with the lo vertex at the same place of the face: a grid of cells at least 2 atol wide over
        # the other coordinates, and a look into the neighbouring cells, so that round-off across a cell border (an
        # imported mesh) cannot separate a pair
        w = np.maximum(np.maximum(2.0 * atol[oth], 2e-9 * span[oth]), 1e-300)
        cl = np.floor((x[il][:, oth] - lo[oth]) / w).astype(np.int64) + 1
        ch = np.floor((x[ih][:, oth] - lo[oth]) / w).astype(np.int64) + 1
        stride = np.int64(max(int(cl.max(initial=0)), int(ch.max(initial=0))) + 3)

        def cell_key(c):
            key = np.zeros(c.shape[0], dtype=np.int64)
            for j in range(c.shape[1]):
                key = key * stride + c[:, j]
            return key
        kl = cell_key(cl)
        srt = np.argsort(kl, kind="stable")
        kls = kl[srt]
        partner = np.full(ih.shape[0], -1, dtype=np.int64)
        for off in itertools.product((-1, 0, 1), repeat=len(oth)):
            kq = cell_key(ch + np.asarray(off, dtype=np.int64))
            p0, p1 = np.searchsorted(kls, kq, side="left"), np.searchsorted(kls, kq, side="right")
            for r in range(int((p1 - p0).max(initial=0))):  # (cells hold one vertex unless vertices nearly coincide)
                cand = np.minimum(p0 + r, kls.shape[0] - 1)
                ok = (p0 + r < p1) & (partner < 0)
                j = srt[cand]
                ok &= (np.abs(x[il[j]][:, oth] - x[ih][:, oth]) <= atol[oth]).all(axis=1)
                partner[ok] = j[ok]
        if (partner < 0).any():
            bad = int(np.argmax(partner < 0))
            raise ValueError(f"make_periodic: axis {k}: the vertices of the two faces do not match (vertex {int(ih[bad])} at "
                             f"{x[ih[bad]].tolist()} has no image on the lo face)")
        if np.unique(partner).shape[0] != partner.shape[0]:
            raise ValueError(f"make_periodic: axis {k}: the vertices of the two faces do not match one to one (two vertices of "
                             "the hi face share an image on the lo face)")
        il = il[partner]
        mk = np.arange(nv, dtype=np.int64)
        mk[ih] = il
        # facets: every facet of the hi face must be, vertex for vertex, a facet of the lo face.  A facet in a face of
        # the bounding box belongs to one cell, which has its other vertex off the face: read from the cells, without the
        # facet table of the whole mesh
        def face_keys(on, relabel):
            c = cells[on[cells].sum(axis=1) == d]  # cells with a facet in the face
            v = np.sort(relabel[c[on[c]].reshape(-1, d)], axis=1)  # (row-major mask: each cell's d face vertices)
            key = np.zeros(v.shape[0], dtype=np.int64)
            for j in range(d):
                key = key * np.int64(nv) + v[:, j]
            return np.sort(key)
        kl, kh = face_keys(on_lo, np.arange(nv, dtype=np.int64)), face_keys(on_hi, mk)
        if kl.shape[0] != kh.shape[0] or (kl != kh).any():
            raise ValueError(f"make_periodic: axis {k}: the facets of the two faces do not match "
                             f"({kl.shape[0]} on the lo face, {kh.shape[0]} on the hi face, "
                             f"{int(np.intersect1d(kl, kh).shape[0])} in common)")
        # three cells across: no vertex may share cells with vertices of both faces
        near_lo, near_hi = np.zeros(nv, dtype=bool), np.zeros(nv, dtype=bool)
        near_lo[cells[on_lo[cells].any(axis=1)].ravel()] = True
        near_hi[cells[on_hi[cells].any(axis=1)].ravel()] = True
        if (near_lo & near_hi).any():
            raise ValueError(f"make_periodic: axis {k}: fewer than three cells across (vertex "
                             f"{int(np.argmax(near_lo & near_hi))} shares cells with both faces): distinct edges would be identified")
        vm = mk[vm]
        masks += [on_lo, on_hi]
    out = Mesh(mesh.coords, mesh.cells, mesh.comm)
    out._ent = dict(mesh._ent)
    out.periodic = PeriodicMap(out, axes, lo, hi, period, atol, vm, masks)
    return out


# ---- entity location and tags ------------------------------------------------------------


def exterior_facet_indices(topology) -> np.ndarray:
    return topology._mesh.exterior_facets()


def _marked_entities(mesh: Mesh, dim: int, marker, candidates=None) -> np.ndarray:
    ev, _ = mesh._entities(dim)
    x = mesh.geometry.x.T  # (3, nv)
    on = np.asarray(marker(x), dtype=bool)
    hit = on[ev].all(axis=1)
    if candidates is not None:
        mask = np.zeros(ev.shape[0], dtype=bool)
        mask[candidates] = True
        hit &= mask
    return np.nonzero(hit)[0].astype(np.int32)


def locate_entities(mesh: Mesh, dim: int, marker) -> np.ndarray:
    """Entities all of whose vertices satisfy ``marker(x)``, x of shape (3, nverts)."""
    return _marked_entities(mesh, dim, marker)


def locate_entities_boundary(mesh: Mesh, dim: int, marker) -> np.ndarray:
    ext = mesh.exterior_facets()
    if dim == mesh.gdim - 1:
        return _marked_entities(mesh, dim, marker, candidates=ext)
    # sub-entities of exterior facets (DOLFINx: entities ATTACHED to a boundary facet -- an interior edge of a tetrahedral
    # mesh whose two end points happen to lie on the boundary is not one of them)
    import itertools

    fv, _ = mesh._entities(mesh.gdim - 1)
    ev, _ = mesh._entities(dim)
    nv = np.int64(mesh.num_vertices)

    def keys(v):
        v = np.sort(np.asarray(v, dtype=np.int64), axis=1)
        k = np.zeros(v.shape[0], dtype=np.int64)
        for c in range(v.shape[1]):
            k = k * nv + v[:, c]
        return k
    sub = np.concatenate([keys(fv[ext][:, list(combo)]) for combo in itertools.combinations(range(fv.shape[1]), dim + 1)])
    cand = np.nonzero(np.isin(keys(ev), np.unique(sub)))[0]
    return _marked_entities(mesh, dim, marker, candidates=cand)


class MeshTags:
    def __init__(self, mesh, dim, indices, values):
        self.mesh = mesh
        self.dim = int(dim)
        self.indices = np.asarray(indices, dtype=np.int32)
        self.values = np.asarray(values)
        self.topology = mesh.topology

    def find(self, value) -> np.ndarray:
        return self.indices[self.values == value]


def meshtags(mesh: Mesh, dim: int, entities, values) -> MeshTags:
    entities = np.asarray(entities)
    if entities.size > 1 and not (np.diff(entities) > 0).all():
        raise RuntimeError("meshtags: entities must be sorted and unique")
    return MeshTags(mesh, dim, entities, values)
