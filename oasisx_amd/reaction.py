"""Reacting scalars: stiff mass-action kinetics between the scalars of ``FractionalStep_AB_CN``, split from the transport
step and integrated per dof on the device (``ox_scalar_react``, csrc/ox_reaction.hip).

The rate of reaction ``j`` at a dof and the source of species ``s``::

    r_j = k_j(x) [exp(-Ta_j / c_T)] prod_s c_s^o_js
    dc_s/dt = sum_j nu_sj r_j,        nu_sj = products_j.get(s, 0) - reactants_j.get(s, 0)

The orders ``o_js`` are integers 0..3 formed by repeated multiplication: no ``pow``, and nothing is ever divided by a
concentration (the Jacobian lowers one factor's order).  The Arrhenius factor divides by its temperature and has NO guard
on ``c_T <= 0``: a value that is not finite stays in its own dof.

The integrator is ROS2 (Verwer, Spee, Blom, Hundsdorfer 1999): second order, L-stable, one LU per substep, the analytic
Jacobian.  With ``g = 1 + 1/sqrt(2)``, ``h = H / substeps`` and ``W = I - g h J(y)``::

    W k1 = f(y);    W k2 = f(y + h k1) - 2 k1;    y <- y + 1.5 h k1 + 0.5 h k2

The step count is fixed (no adaptivity): equal inputs give equal bits.  There is no positivity clipping.

Splitting (``FractionalStep_AB_CN.solve``):

``"strang"`` (default)
    ``scalar_react(dt/2)`` on ``c_1`` before ``assemble_first`` -- the scalar operator's right-hand side, SUPG's right-hand
    side and the buoyancy force see the reacted level; ``c_2`` of an extrapolating scalar stays the previous step's end
    value --, the unchanged transport step, ``scalar_react(dt/2)`` on its result.  Splitting error ``O(dt^2)``.
``"lie"``
    one ``scalar_react(dt)`` after ``scalar_solve``.  Splitting error ``O(dt)``.

After either, ``scalar(name)`` and ``scalar(name, level=1)`` hold the same reacted bits.  A species' own Dirichlet rows
keep their boundary value bit for bit; that value still enters the rates of the other species at the dof (the held species
is integrated with the others and its result is not written).  Reaction is nodal: the kinetics act on the dof values, no
mass matrix is involved.  One GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .fem import FieldStorage, Function

__all__ = ["Reaction", "ReactionNetwork"]

MAX_SPECIES, MAX_REACTIONS = _lib.REACT_MAXS, _lib.REACT_MAXR  # OX_REACT_MAXS, OX_REACT_MAXR
SPLITTINGS = ("strang", "lie")


def _coefficients(who, what, d):
    """``{name: coefficient}`` with real, finite coefficients >= 0."""
    if d is None:
        return {}
    if not isinstance(d, dict):
        raise TypeError(f"{who}: {what} is a dict name -> coefficient (got {type(d).__name__})")
    out = {}
    for name, v in d.items():
        if not isinstance(name, str) or not name:
            raise ValueError(f"{who}: {what}: species names are non-empty strings (got {name!r})")
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: {what}[{name!r}] = {v!r}: a finite float >= 0 is expected") from None
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(f"{who}: {what}[{name!r}] = {v}: a finite float >= 0 is expected")
        out[name] = v
    return out


class Reaction:
    """One reaction ``sum_s reactants[s] s -> sum_s products[s] s`` with the mass-action rate of the module docstring.

    Args:
        rate: ``k``: a finite float >= 0, a callable ``f(x)`` on ``x: (3, npts)`` or a ``Function`` on the solver's
            component space, evaluated once at the dofs (a catalytic region, a zone with no reaction);
            ``ReactionNetwork.update()`` re-evaluates the callables
        reactants: ``{name: coefficient}``, real, finite, >= 0
        products: ``{name: coefficient}``; a real coefficient on a temperature scalar is the heat release
        orders: ``None``: the orders are the reactant coefficients, which must then be integers 0..3; a dict
            ``{name: order}`` states them independently of the stoichiometry (names left out have order 0)
        arrhenius: ``None`` or ``(name, Ta)``: the rate is multiplied by ``exp(-Ta / c_name)`` (no guard on ``c_name <= 0``)
    """

    def __init__(self, rate, reactants, products=None, orders=None, arrhenius=None):
        who = "Reaction"
        if callable(rate) or isinstance(rate, Function):
            self.rate = rate
        else:
            try:
                k = float(rate)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: rate = {rate!r}: a finite float >= 0, a callable f(x) or a Function is "
                                 "expected") from None
            if not (np.isfinite(k) and k >= 0.0):
                raise ValueError(f"{who}: rate = {k}: a finite float >= 0 is expected")
            self.rate = k
        self.reactants = _coefficients(who, "reactants", reactants)
        self.products = _coefficients(who, "products", products)
        if not self.reactants and not self.products:
            raise ValueError(f"{who}: neither reactants nor products")
        if orders is None:
            self.orders = {}
            for name, v in self.reactants.items():
                if v != int(v) or not 0 <= int(v) <= 3:
                    raise ValueError(f"{who}: the reactant coefficient {v} of {name!r} is no integer order 0..3: state "
                                     "orders={...} beside the stoichiometry")
                self.orders[name] = int(v)
        else:
            if not isinstance(orders, dict):
                raise TypeError(f"{who}: orders is a dict name -> order (got {type(orders).__name__})")
            self.orders = {}
            for name, o in orders.items():
                if not isinstance(name, str) or not name:
                    raise ValueError(f"{who}: orders: species names are non-empty strings (got {name!r})")
                if isinstance(o, (bool, np.bool_)) or not isinstance(o, (int, np.integer)) or not 0 <= int(o) <= 3:
                    raise ValueError(f"{who}: orders[{name!r}] = {o!r}: an integer 0..3 is expected")
                self.orders[name] = int(o)
        self.arrhenius = None
        if arrhenius is not None:
            try:
                name, Ta = arrhenius
                Ta = float(Ta)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: arrhenius = {arrhenius!r}: (scalar_name, Ta) is expected") from None
            if not isinstance(name, str) or not name or not np.isfinite(Ta):
                raise ValueError(f"{who}: arrhenius = {arrhenius!r}: (scalar_name, Ta) with a finite Ta is expected")
            self.arrhenius = (name, Ta)

    def names(self):
        """The species the reaction names, in the order reactants, products, orders, Arrhenius temperature."""
        out = list(self.reactants) + list(self.products) + list(self.orders)
        if self.arrhenius is not None:
            out.append(self.arrhenius[0])
        return list(dict.fromkeys(out))

    def key(self):
        """What makes two reactions the same one."""
        rate = ("float", self.rate) if isinstance(self.rate, float) else ("object", id(self.rate))
        return (rate, tuple(sorted(self.reactants.items())), tuple(sorted(self.products.items())),
                tuple(sorted((n, o) for n, o in self.orders.items() if o)), self.arrhenius)

    def __repr__(self):
        return (f"Reaction({self.rate!r}, reactants={self.reactants}, products={self.products}, orders={self.orders}, "
                f"arrhenius={self.arrhenius})")


class ReactionNetwork:
    """The reactions between the scalars of one solver, ``FractionalStep_AB_CN(..., scalars=[...], reactions=network)``.

    Args:
        reactions: a list of 1..12 :class:`Reaction` between at most 6 species (``NotImplementedError`` beyond: the kernel
            keeps the ``S x S`` matrix of a dof in registers); a reaction listed twice raises ``ValueError``
        substeps: ROS2 steps per ``scalar_react`` call (an int >= 1; fixed, there is no adaptivity)
        splitting: ``"strang"`` (default, ``O(dt^2)``) or ``"lie"`` (``O(dt)``): the module docstring

    ``species``: the names that occur in any reaction, in the order of first appearance; a scalar of the solver named
    nowhere is never read or written.
    """

    def __init__(self, reactions, substeps: int = 1, splitting: str = "strang"):
        reactions = list(reactions)
        if not reactions:
            raise ValueError("ReactionNetwork: no reactions")
        for r in reactions:
            if not isinstance(r, Reaction):
                raise TypeError(f"ReactionNetwork: reactions holds Reaction objects (got {type(r).__name__})")
        keys = [r.key() for r in reactions]
        for i, k in enumerate(keys):
            if k in keys[:i]:
                raise ValueError(f"ReactionNetwork: duplicate reaction {reactions[i]!r}")
        if isinstance(substeps, (bool, np.bool_)) or not isinstance(substeps, (int, np.integer)) or int(substeps) < 1:
            raise ValueError(f"ReactionNetwork: substeps = {substeps!r}: an int >= 1 is expected")
        if splitting not in SPLITTINGS:
            raise ValueError(f'ReactionNetwork: splitting = {splitting!r}: "strang" or "lie" is expected')
        self.reactions, self.substeps, self.splitting = reactions, int(substeps), splitting
        self.species = list(dict.fromkeys(n for r in reactions for n in r.names()))
        if len(self.species) > MAX_SPECIES:
            raise NotImplementedError(f"ReactionNetwork: {len(self.species)} species {self.species}: the kernel is built "
                                      f"for at most {MAX_SPECIES} (OX_REACT_MAXS)")
        if len(reactions) > MAX_REACTIONS:
            raise NotImplementedError(f"ReactionNetwork: {len(reactions)} reactions: the kernel's record holds at most "
                                      f"{MAX_REACTIONS} (OX_REACT_MAXR)")
        self._solver = None

    # ---- host tables -----------------------------------------------------------------------------------------------------
    def stoichiometry(self) -> np.ndarray:
        """``nu``: (n_species, n_reactions), products minus reactants."""
        nu = np.zeros((len(self.species), len(self.reactions)))
        for j, r in enumerate(self.reactions):
            for s, name in enumerate(self.species):
                nu[s, j] = r.products.get(name, 0.0) - r.reactants.get(name, 0.0)
        return nu

    def orders(self) -> np.ndarray:
        """(n_reactions, n_species) integers 0..3."""
        o = np.zeros((len(self.reactions), len(self.species)), dtype=np.int32)
        for j, r in enumerate(self.reactions):
            for s, name in enumerate(self.species):
                o[j, s] = r.orders.get(name, 0)
        return o

    def arrhenius(self):
        """Per reaction ``(index of the temperature species | -1, Ta)``."""
        return [(-1, 0.0) if r.arrhenius is None else (self.species.index(r.arrhenius[0]), r.arrhenius[1])
                for r in self.reactions]

    def invariants(self) -> np.ndarray:
        """An orthonormal basis of the left null space of ``nu``, (n_invariants, n_species): every row ``w`` has
        ``w^T nu = 0``, so ``sum_s w_s c_s`` is kept by the kinetics at every dof (computed on the host, by an SVD)."""
        nu = self.stoichiometry()
        u, sv, _ = np.linalg.svd(nu, full_matrices=True)
        tol = max(nu.shape) * np.finfo(np.float64).eps * (sv[0] if sv.size else 0.0)
        rank = int((sv > tol).sum())
        return np.ascontiguousarray(u[:, rank:].T)

    # ---- the solver's side ---------------------------------------------------------------------------------------------
    def check_names(self, names) -> None:
        """Every species is one of the solver's scalars (run before the library is loaded)."""
        unknown = [s for s in self.species if s not in names]
        if unknown:
            raise ValueError(f"ReactionNetwork: unknown species {unknown}: the solver's scalars are {sorted(names)}")

    def bind(self, solver) -> None:
        """The kernel's records for ``solver``: the network by value, per species the block its group keeps it in, the byte
        mask of its Dirichlet rows, and one device column per rate that is not a float."""
        if self._solver is not None and self._solver is not solver:
            raise ValueError("ReactionNetwork: the network belongs to another solver already")
        self.check_names(solver._scalar_index)
        self._solver = solver
        Vi = solver._Vi[0][0]
        dev = solver._mesh.device
        n = solver._n_u
        S, R = len(self.species), len(self.reactions)
        net = _lib.ox_react_net()
        net.S, net.R = S, R
        nu, orders = self.stoichiometry(), self.orders()
        for s in range(S):
            for j in range(R):
                net.nu[s][j] = nu[s, j]
                net.order[j][s] = int(orders[j, s])
        self._fields = [j for j, r in enumerate(self.reactions) if not isinstance(r.rate, float)]
        self._K = {j: FieldStorage(n, 1, dev) for j in self._fields}  # (n, 1) each: the kernel reads them with stride 1
        self._k = {j: Function(Vi, f"k_{j}", self._K[j], 0) for j in self._fields}
        for j, (r, (a, Ta)) in enumerate(zip(self.reactions, self.arrhenius())):
            net.k[j] = r.rate if isinstance(r.rate, float) else 0.0
            net.arr[j], net.Ta[j] = a, Ta
            if isinstance(r.rate, Function) and getattr(r.rate.function_space, "scalar", r.rate.function_space) is not Vi:
                raise ValueError(f"{r!r}: a Function rate must live on the velocity component space")
        self._net = net
        self._groups = [solver._scalar_index[name] for name in self.species]
        self._held = {}
        for g, _ in self._groups:  # the group's Dirichlet rows as a byte mask, one per group with such rows
            if id(g) not in self._held and g.rows_dev.shape[0] > 0:
                mask = torch.zeros(n, dtype=torch.uint8, device=dev)
                mask[g.rows_dev.to(torch.int64)] = 1
                self._held[id(g)] = mask
        self._species = (_lib.ox_react_species * S)()
        for t, (g, col) in zip(self._species, self._groups):
            t.nc, t.col = g.nc, col
            held = self._held.get(id(g))
            t.held = None if held is None else held.data_ptr()
        self._rates = torch.zeros((R, n), dtype=torch.float64, device=dev)
        self.update(first=True)

    def update(self, first: bool = False) -> None:
        """Re-evaluate the callable rates at the dofs (``FractionalStep_AB_CN.solve`` calls it where it calls
        ``update_bc``); a ``Function`` rate is copied once, at construction.  A rate that is negative or not finite at a dof
        raises ``ValueError``."""
        if self._solver is None:
            raise RuntimeError("ReactionNetwork.update: the network has not been handed to a solver (reactions=)")
        for j in self._fields:
            f = self.reactions[j].rate
            if isinstance(f, Function):
                if not first:
                    continue
                self._K[j].dev()[:, 0] = f._storage.rdev()[:, 0 if f._comp is None else f._comp]
            else:
                self._k[j].interpolate(f)
            v = self._K[j].rhost()[:, 0]
            if not (np.isfinite(v).all() and (v >= 0.0).all()):
                raise ValueError(f"{self.reactions[j]!r}: the rate is negative or not finite at a dof")

    def _records(self, write: bool):
        """(network, species) for one launch: the blocks' current device pointers (a block checked out to the host goes
        back first).  ``write``: c_1 is read, c_1 and c are written; otherwise c is read through ``rptr()``."""
        for j in self._fields:
            self._net.kdof[j] = self._K[j].rptr().value
        ptrs = {}
        for g, _ in self._groups:
            if id(g) not in ptrs:
                ptrs[id(g)] = (g.C1.ptr().value, g.C.ptr().value) if write else (g.C.rptr().value, None)
        for t, (g, _) in zip(self._species, self._groups):
            a, b = ptrs[id(g)]
            t.src, t.out, t.out2 = a, a if write else None, b
        return self._net, self._species

    def react(self, h: float) -> None:
        """``substeps`` ROS2 steps over ``h`` from ``c_1`` into ``c_1`` and ``c``: one launch, no host synchronisation."""
        S = self._solver
        net, sp = self._records(True)
        _lib.check(S._lib.ox_scalar_react(C.byref(net), sp, int(S._n_u), float(h), self.substeps, _lib.current_stream()),
                   "ox_scalar_react")

    def rates(self) -> torch.Tensor:
        """``r_j`` of the current level ``c``: (n_reactions, n_dofs) on the device, a rate-only launch."""
        S = self._solver
        net, sp = self._records(False)
        _lib.check(S._lib.ox_reaction_rates(C.byref(net), sp, int(S._n_u), _lib.ptr(self._rates), _lib.current_stream()),
                   "ox_reaction_rates")
        return self._rates
