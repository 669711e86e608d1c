"""Lagrangian tracers at sizes a user runs: Taylor-Green 128^3, P2-P1, one GPU.

    python tools/tracer_bench.py [-N 128] [--particles 1000000] [--lattice 100] [--reps 20] [--warmup 10] [--out FILE]

(i)   ``Tracers.advance`` (RK4, substeps = 1) of ``--particles`` particles seeded uniformly at random and, separately, on
      a ``--lattice``^3 lattice, after ``--warmup`` time steps: device events around ``--reps`` advances, median and mean
      (the mean counts the re-sort of ``sort_every`` = 8, which the median hides), for hint on / off and sort_every 0, 1, 8.
      Particles/s and bytes/s over the bytes a step NEEDS, computed from the shapes (per stage: the cell's first vertex
      and gradients, its kernel position, nd indices and nd rows of nc doubles of both levels; per advance: the end
      point's cell and the particle state in and out), as a share of the 8 TB/s peak -- a gather kernel's share.
(ii)  the composed path the kernel replaces, in the same process on the same seeds: per stage ``tree.find`` +
      ``PointPlan`` + 2 x ``ox_eval_points`` + torch axpys (no freeze rule, no age / path: every advantage).
(iii) ``--steps`` time steps with and ``--steps`` without an advance of the random particles, alternating.
One JSON line per case on stdout (and appended to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_BYTES_PER_S = 8.0e12


def seeds(W, kind, n, lattice):
    import numpy as np

    q0, q1 = np.asarray(W["box"][0], dtype=np.float64), np.asarray(W["box"][1], dtype=np.float64)
    if kind == "random":
        return q0 + (q1 - q0) * (0.03 + 0.94 * np.random.default_rng(0).random((n, 3)))
    ax = [np.linspace(q0[k] + 0.03 * (q1[k] - q0[k]), q1[k] - 0.03 * (q1[k] - q0[k]), lattice) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def ms(np, evs):
    return np.asarray([a.elapsed_time(b) for a, b in evs])


def bytes_per_advance(nd, nc, stages=4):
    cell = 8 * (3 + 9)  # first vertex and gradients of one tetrahedron
    stage = cell + 8 + nd * 4 + 2 * nd * nc * 8
    state = 2 * (3 * 8 + 8 + 4 + 3 * 8)  # x, cell, status, age / path / exit time: in and out
    return stages * stage + cell + state


def case_advance(S, W, kind, x, reps, hint, sort_every):
    import numpy as np
    import torch

    import oasisx_amd as ox
    from probe_bench import timed

    T = ox.Tracers(S, x, scheme="rk4", substeps=1, hint=hint, sort_every=sort_every)
    for _ in range(2):
        T.advance(W["dt"])
    evs = [timed(torch, lambda: T.advance(W["dt"]))[0] for _ in range(reps)]
    torch.cuda.synchronize()
    t = ms(np, evs)
    n, nd, nc = T.n, int(T.Vs.cell_dofs.shape[1]), S._U1.nc
    b = bytes_per_advance(nd, nc)
    med = float(np.median(t))
    return {"case": "advance", "seeds": kind, "particles": n, "hint": hint, "sort_every": sort_every, "scheme": "rk4",
            "advance_ms_median": med, "advance_ms_mean": float(t.mean()), "advance_ms_max": float(t.max()),
            "particles_per_s": n / (med * 1e-3), "particles_per_s_mean": n / (float(t.mean()) * 1e-3),
            "bytes_needed_per_particle_stage": b / 4.0, "bytes_per_s": n * b / (med * 1e-3),
            "share_of_8TBps_peak_gather_kernel": n * b / (med * 1e-3) / PEAK_BYTES_PER_S,
            "alive": int((T.status() == 0).sum())}, T


def case_composed(S, W, kind, x, reps, fused):
    """Four RK4 stages through the public pieces; ``fused``: a Tracers object advanced the same number of times from the
    same seeds, for the deviation."""
    import numpy as np
    import torch

    from oasisx_amd import _lib
    from oasisx_amd import geometry as G
    from probe_bench import timed

    Vs = G.scalar_space(S.u.function_space)
    tree = G.space_tree(Vs)
    lib, st = _lib.load(), _lib.current_stream()
    X = torch.from_numpy(x).to(S._U.rdev().device)
    n, nc = int(X.shape[0]), S._U1.nc
    va, vb = (torch.empty((n, nc), dtype=torch.float64, device=X.device) for _ in range(2))

    def velocity(xs, theta):
        cells, bary = tree.find(xs)
        plan = G.PointPlan(Vs, cells, bary)
        for blk, out in ((S._U2, va), (S._U1, vb)):
            _lib.check(lib.ox_eval_points(*plan.args(), blk.rptr(), nc, -1, _lib.ptr(out), nc, 0, st), "ox_eval_points")
        return va + theta * (vb - va)

    def advance(X, h):
        k1 = velocity(X, 0.0)
        k2 = velocity(X + 0.5 * h * k1, 0.5)
        k3 = velocity(X + 0.5 * h * k2, 0.5)
        k4 = velocity(X + h * k3, 1.0)
        return X + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)

    state = {"X": X}

    def one():
        state["X"] = advance(state["X"], W["dt"])

    for _ in range(2):
        one()
    evs = [timed(torch, one)[0] for _ in range(reps)]
    torch.cuda.synchronize()
    t = ms(np, evs)
    dev = float((state["X"] - torch.from_numpy(fused.positions()).to(X.device)).abs().max())
    return {"case": "composed", "seeds": kind, "particles": n, "advance_ms_median": float(np.median(t)),
            "advance_ms_mean": float(t.mean()), "particles_per_s": n / (float(np.median(t)) * 1e-3),
            "max_abs_composed_minus_fused": dev}


def case_steps(S, W, clk, x, steps):
    import numpy as np
    import torch

    import oasisx_amd as ox
    from probe_bench import timed

    T = ox.Tracers(S, x, scheme="rk4", substeps=1)
    plain, traced, alone = [], [], []
    for k in range(2 * steps):
        clk["t"] += W["dt"]
        if k % 2 == 0:
            plain.append(timed(torch, lambda: S.solve(W["dt"], W["nu"], max_iter=1))[0])
        else:
            def both():
                S.solve(W["dt"], W["nu"], max_iter=1)
                alone.append(timed(torch, lambda: T.advance(W["dt"]))[0])
            traced.append(timed(torch, both)[0])
    torch.cuda.synchronize()
    p, q, a = ms(np, plain), ms(np, traced), ms(np, alone)
    return {"case": "steps", "particles": T.n, "steps_each": steps, "plain_step_ms_mean": float(p.mean()),
            "plain_step_ms_std": float(p.std()), "traced_step_ms_mean": float(q.mean()),
            "added_ms_per_step": float(q.mean() - p.mean()), "advance_alone_ms_mean": float(a.mean()),
            "alive": int((T.status() == 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--lattice", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from probe_bench import build

    S, W, clk, mesh = build(a.N)
    for _ in range(a.warmup):
        clk["t"] += W["dt"]
        S.solve(W["dt"], W["nu"], max_iter=1)

    def emit(r):
        r["mesh_N"] = a.N
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    best = {}
    for kind in ("random", "lattice"):
        x = seeds(W, kind, a.particles, a.lattice)
        plain = None
        for hint in (True, False):
            for sort_every in (0, 1, 8):
                r, T = case_advance(S, W, kind, x, a.reps, hint, sort_every)
                emit(r)
                if hint and sort_every == 0:
                    plain = T
                best[kind] = min(best.get(kind, float("inf")), r["advance_ms_mean"])
        c = case_composed(S, W, kind, x, a.reps, plain)
        c["fused_best_ms_mean"] = best[kind]
        c["fused_beats_composed"] = bool(best[kind] < c["advance_ms_mean"])
        emit(c)
    emit(case_steps(S, W, clk, seeds(W, "random", a.particles, a.lattice), a.steps))
    return 0


if __name__ == "__main__":
    sys.exit(main())
