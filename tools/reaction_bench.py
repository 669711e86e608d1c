"""Reacting scalars at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm start): ONE solver, one process, HIP
events, medians, the versions alternating inside the timed loop.

    python tools/reaction_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out FILE]

Part 1, the kernels, launch after launch, alternating:
  ``ox_scalar_react`` with 2 / 4 / 6 species (a decay chain plus one bimolecular step: S + 1 reactions; the species in
  interleaved blocks of two columns, written to two levels as the solver does) at ``substeps`` 1 and 4, each beside
  ``ox_axpby`` on the same bytes (S columns read, 2 S columns written: the bandwidth yardstick) and beside
  ``ox_scalar_rows`` of one scalar group of three columns (what the transport step pays per group anyway);
  ``ox_reaction_rates`` of the six-species network.
  Bytes moved per launch: 8 B per dof and species read, 16 B written.
Part 2, the step: ms per step with a three-species network ``A + B -> C`` (Strang: two launches per step) switched on and
  off from step to step (the species are passive, so both variants follow the same flow), ``scalar_react`` split out."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s


def build(N):
    import numpy as np
    import torch

    import oasisx_amd as ox
    from bench import make_workload
    from oasisx_amd import mesh as M

    W = make_workload("tg", N, np, torch)
    q0, q1 = W["box"]
    clk = {"t": 0.0}

    def on_bnd(x):
        on = np.zeros(x.shape[1], dtype=bool)
        for k in range(3):
            on |= np.isclose(x[k], q0[k]) | np.isclose(x[k], q1[k])
        return on

    def at(f, t):
        def g(x):
            return f(x, clk["t"] if t is None else t)
        g.supports_torch = True
        return g

    mesh = M.create_box(None, [q0, q1], [N, N, N])
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
    G = ox.LocatorMethod.GEOMETRICAL
    ini = {"A": lambda x: 1.0 + 0.5 * np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]), "B": lambda x: 0.8 + 0.3 * np.sin(np.pi * x[2]),
           "C": lambda x: 0.1 + 0.0 * x[0]}
    scalars = [ox.ScalarTransport(n, schmidt=1.0, initial=ini[n]) for n in "ABC"]
    net = ox.ReactionNetwork([ox.Reaction(5.0, {"A": 1, "B": 1}, {"C": 1})])
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(at(f, None), G, on_bnd)] for f in W["fns"]], bcs_p=[],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg")}, options={}, scalars=scalars,
                                reactions=net)
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    return S, W, clk


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def chain_network(_lib, ns, blocks_in, blocks_out, blocks_out2):
    """A decay chain s0 -> s1 -> ... -> (nothing) plus s0 + s1 -> (s2 | s1): the kernel's records on blocks of two columns."""
    net = _lib.ox_react_net()
    net.S, net.R = ns, ns + 1
    for j in range(ns):
        net.k[j], net.arr[j] = 0.5 + 0.25 * j, -1
        net.order[j][j] = 1
        net.nu[j][j] = -1.0
        if j + 1 < ns:
            net.nu[j + 1][j] = 1.0
    j = ns
    net.k[j], net.arr[j] = 1.5, -1
    net.order[j][0] = net.order[j][1] = 1
    net.nu[0][j] = net.nu[1][j] = -1.0
    net.nu[2 if ns > 2 else 1][j] += 1.0
    sp = (_lib.ox_react_species * ns)()
    for s in range(ns):
        sp[s].src, sp[s].out, sp[s].out2 = (b[s // 2].data_ptr() for b in (blocks_in, blocks_out, blocks_out2))
        sp[s].nc, sp[s].col = 2, s % 2
    return net, sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--steps", type=int, default=12, help="timed steps per variant")
    ap.add_argument("--warmup", type=int, default=4, help="warm-up steps (network on)")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from oasisx_amd import _lib

    S, W, clk = build(a.N)
    dt, nu = W["dt"], W["nu"]
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()

    # ---- part 1: the kernels ---------------------------------------------------------------------------------------
    lib, st = _lib.load(), _lib.current_stream()
    n = int(S._n_u)
    dev = S._mesh.device
    gen = torch.Generator(device="cpu").manual_seed(1)
    src = [(0.1 + torch.rand((n, 2), dtype=torch.float64, generator=gen)).to(dev) for _ in range(3)]
    out = [torch.zeros_like(b) for b in src]
    out2 = [torch.zeros_like(b) for b in src]
    flat_in = torch.zeros(6 * n, dtype=torch.float64, device=dev)
    flat_out = torch.zeros(12 * n, dtype=torch.float64, device=dev)
    rates = torch.zeros((7, n), dtype=torch.float64, device=dev)
    nets = {ns: chain_network(_lib, ns, src, out, out2) for ns in (2, 4, 6)}
    g = S._scalar_groups[0]
    assert g.nc == 3
    P = S._M.pattern

    def react(ns, substeps):
        net, sp = nets[ns]
        _lib.check(lib.ox_scalar_react(C.byref(net), sp, n, dt, substeps, st), "ox_scalar_react")

    def axpby(ns):  # ns n doubles read, 2 ns n written: the same bytes as the kernel with two output levels
        _lib.check(lib.ox_axpby(ns * n, 1.0, _lib.ptr(flat_in), 0.0, None, _lib.ptr(flat_out), st), "ox_axpby")
        _lib.check(lib.ox_axpby(ns * n, 1.0, _lib.ptr(flat_in), 0.0, None, C.c_void_p(flat_out.data_ptr() + 8 * ns * n), st),
                   "ox_axpby")

    def rows():
        _lib.check(lib.ox_scalar_rows(S._A.ref(), S._M.ref(), S._K.ref(), g.Ac.ref(), 0.0, float(dt), g.nc, g.C1.rptr(),
                                      g.B0.rptr(), g.B.ptr(), None, st), "ox_scalar_rows")

    def rates6():
        net, sp = nets[6]
        _lib.check(lib.ox_reaction_rates(C.byref(net), sp, n, _lib.ptr(rates), st), "ox_reaction_rates")

    variants = {}
    for ns in (2, 4, 6):
        for sub in (1, 4):
            variants[f"scalar_react_{ns}_substeps_{sub}"] = lambda ns=ns, sub=sub: react(ns, sub)
        variants[f"axpby_{ns}"] = lambda ns=ns: axpby(ns)
    variants["scalar_rows_3_columns"] = rows
    variants["reaction_rates_6"] = rates6
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4)}
        ns = int(k.split("_")[2]) if k.startswith("scalar_react") else int(k.split("_")[1]) if k.startswith("axpby") else 0
        if ns:
            kern[k]["bytes"] = 24 * ns * n
            kern[k]["fraction_of_hbm_peak"] = round(24 * ns * n / (ms * 1e-3) / HBM_PEAK, 4)
    for ns in (2, 4, 6):
        for sub in (1, 4):
            kern[f"react_over_axpby_{ns}_substeps_{sub}"] = round(kern[f"scalar_react_{ns}_substeps_{sub}"]["ms"]
                                                                 / kern[f"axpby_{ns}"]["ms"], 3)

    # ---- part 2: whole steps, the network on and off alternating ----------------------------------------------------
    phase = []
    inner = S.scalar_react

    def wrapped(h):
        phase.append(timed(torch, lambda: inner(h)))

    S.scalar_react = wrapped
    sets = {"without": None, "with_network": S._reactions}
    rec = {k: {"step": [], "react": []} for k in sets}
    for i in range(a.steps + 1):
        for k, rx in sets.items():
            S._reactions = rx
            phase.clear()
            clk["t"] += dt
            e = timed(torch, lambda: S.solve(dt, nu, max_iter=1))
            torch.cuda.synchronize()
            if i == 0:
                continue
            rec[k]["step"].append(e[0].elapsed_time(e[1]))
            rec[k]["react"].append(sum(x.elapsed_time(y) for x, y in phase))
    steps = {k: {"ms_per_step": round(statistics.median(v["step"]), 3),
                 "min_ms": round(min(v["step"]), 3), "max_ms": round(max(v["step"]), 3),
                 "scalar_react_ms": round(statistics.median(v["react"]), 4)} for k, v in rec.items()}
    res = {"N": a.N, "rows_u": n, "entry_slots": int(P.size), "scalars": 3, "react_launches_per_step": 2, "kernel": kern,
           "steps": steps}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
