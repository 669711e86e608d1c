"""Inertial particles beside the tracers at sizes a user runs: Taylor-Green 128^3, P2-P1, one GPU, one process.

    python tools/particle_bench.py [-N 128] [--particles 1000000] [--reps 20] [--warmup 10] [--steps 20] [--out FILE]
                                   [--bench-trees this=DIR parent=DIR] [--bench-runs 2] [--only-bench]

(i)   ``InertialParticles.advance`` (exp1, exp2; Stokes and Schiller-Naumann) and ``Tracers.advance`` (euler, rk2) on the
      same seeds and the same two levels of the solver, substeps = 1, alternating inside one loop; device events around
      every advance, medians of ``--reps``.  The stage counts, locates and gathers of exp1 / euler and of exp2 / rk2 are
      equal; the particles carry more state and evaluate exp / expm1 (and pow).  Bytes per particle-stage are the bytes a
      stage NEEDS, computed from the shapes (``bytes_per_advance``), and their rate is a gather kernel's share of 8 TB/s.
(ii)  the classification path: one advance of fresh particle sets of which none, and of which about 10 %, leave the mesh in
      that advance (a tenth of the seeds start with a velocity that ends 1 % of the box width outside the face x = hi);
      events around the advance (both launches), medians of ``--reps`` fresh sets each, alternating.  Three more sets whose
      tenth ends TWO BOX WIDTHS outside: there the ring walk finds no bound before it has covered the whole grid.
(iii) ``--steps`` time steps with and ``--steps`` without an exp2 advance, alternating: the time added to a step.
(iv)  ``--bench-trees``: ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees (this commit,
      the parent commit), alternating: the default step makes no new call and must not change.
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
STAGES = {"euler": 1, "rk2": 2, "exp1": 1, "exp2": 2}


def bytes_per_advance(nd, nc, stages, particle):
    """The bytes one advance of one particle needs (3-D): per stage the cell's first vertex and gradients, its kernel
    position, nd indices and nd rows of nc doubles of both levels; the end point's cell; the state in and out."""
    cell = 8 * (3 + 9)
    stage = cell + 8 + nd * 4 + 2 * nd * nc * 8
    state = 2 * (3 * 8 + 8 + 4 + 3 * 8)  # x, cell, status, age / path / exit time
    if particle:
        state += 2 * (3 * 8 + 3 * 4) + 3 * 8 + 4  # v and wraps in and out; tau_p, diameter, beta in; facet (second launch)
    return stages * stage + cell + state


def ms(np, evs):
    return np.asarray([a.elapsed_time(b) for a, b in evs])


def make(S, W, x, scheme, drag="stokes", velocities=None, tau=None):
    import oasisx_amd as ox

    if scheme in ("euler", "rk2"):
        return ox.Tracers(S, x, scheme=scheme, substeps=1)
    tau = 10.0 * W["dt"] if tau is None else tau
    diameter = (18.0 * W["nu"] * tau / 1000.0) ** 0.5
    return ox.InertialParticles(S, x, diameter, 1000.0, fluid_density=1.0, nu=W["nu"], gravity=(0.0, 0.0, -1.0), drag=drag,
                                scheme=scheme, substeps=1, velocities=velocities)


def case_advance(S, W, x, reps, emit):
    import numpy as np
    import torch

    from probe_bench import timed

    names = [("euler", None), ("exp1", "stokes"), ("rk2", None), ("exp2", "stokes"), ("exp1", "schiller_naumann"),
             ("exp2", "schiller_naumann")]
    objs = [make(S, W, x, s, d or "stokes") for s, d in names]
    for o in objs:
        for _ in range(2):
            o.advance(W["dt"])
    evs = [[] for _ in objs]
    for _ in range(reps):
        for k, o in enumerate(objs):
            evs[k].append(timed(torch, lambda o=o: o.advance(W["dt"]))[0])
    torch.cuda.synchronize()
    med = {}
    nd, nc = int(objs[0].Vs.cell_dofs.shape[1]), S._U1.nc
    for (scheme, drag), o, e in zip(names, objs, evs):
        t = ms(np, e)
        m = float(np.median(t))
        med[(scheme, drag)] = m
        b = bytes_per_advance(nd, nc, STAGES[scheme], drag is not None)
        emit({"case": "advance", "scheme": scheme, "drag": drag, "particles": o.n, "advance_ms_median": m,
              "advance_ms_min": float(t.min()), "advance_ms_max": float(t.max()), "particles_per_s": o.n / (m * 1e-3),
              "bytes_needed_per_particle_stage": b / STAGES[scheme], "bytes_needed_per_particle": b,
              "bytes_per_s": o.n * b / (m * 1e-3), "share_of_8TBps_peak_gather_kernel": o.n * b / (m * 1e-3) / PEAK_BYTES_PER_S,
              "alive": int((o.status() == 0).sum())})
    emit({"case": "ratios", "exp1_over_euler": med[("exp1", "stokes")] / med[("euler", None)],
          "exp2_over_rk2": med[("exp2", "stokes")] / med[("rk2", None)],
          "exp2_schiller_naumann_over_stokes": med[("exp2", "schiller_naumann")] / med[("exp2", "stokes")],
          "state_bytes_particle_over_tracer_exp2": bytes_per_advance(nd, nc, 2, True) / bytes_per_advance(nd, nc, 2, False)})


def case_classification(S, W, x, reps, emit):
    import numpy as np
    import torch

    from probe_bench import timed

    q0, q1 = np.asarray(W["box"][0], dtype=np.float64), np.asarray(W["box"][1], dtype=np.float64)
    n = x.shape[0]
    pick = np.random.default_rng(1).random(n) < 0.1
    stay, near, far = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    near[pick, 0] = (q1[0] - x[pick, 0] + 0.01 * (q1[0] - q0[0])) / W["dt"]  # ends 1 % of the box (1.3 cells) outside
    far[pick, 0] = 2.0 * (q1[0] - q0[0]) / W["dt"]  # ends two box widths outside: the ring walk covers the whole grid
    cases = {"none": stay, "tenth": near, "tenth_far": far}
    evs, left = {k: [] for k in cases}, {}
    for r in range(reps + 2):
        for name, v in cases.items():
            if name == "tenth_far" and r >= 5:
                continue
            P = make(S, W, x, "exp2", velocities=v, tau=1e3 * W["dt"])  # (heavy: they keep their velocity)
            torch.cuda.synchronize()
            e = timed(torch, lambda P=P: P.advance(W["dt"]))[0]
            if r >= 2:
                evs[name].append(e)
            left[name] = P
    torch.cuda.synchronize()
    t = {k: ms(np, v) for k, v in evs.items()}
    med = {k: float(np.median(v)) for k, v in t.items()}
    emit({"case": "classification", "particles": n, "left_fraction": float((left["tenth"].status() != 0).mean()),
          "left_fraction_none": float((left["none"].status() != 0).mean()),
          "left_fraction_far": float((left["tenth_far"].status() != 0).mean()), "advance_ms_median_none_leave": med["none"],
          "advance_ms_median_tenth_leaves": med["tenth"], "added_ms": med["tenth"] - med["none"],
          "advance_ms_median_tenth_leaves_two_box_widths_out": med["tenth_far"], "reps_far": int(t["tenth_far"].shape[0]),
          "spread_ms_none": float(t["none"].max() - t["none"].min()), "spread_ms_tenth": float(t["tenth"].max() - t["tenth"].min()),
          "note": "fresh particle sets: every advance timed here is an object's first and includes its sort"})


def case_steps(S, W, clk, x, steps, emit):
    import numpy as np
    import torch

    from probe_bench import timed

    P = make(S, W, x, "exp2")
    plain, laden, alone = [], [], []
    for k in range(2 * steps):
        clk["t"] += W["dt"]
        if k % 2 == 0:
            plain.append(timed(torch, lambda: S.solve(W["dt"], W["nu"], max_iter=1))[0])
        else:
            def both():
                S.solve(W["dt"], W["nu"], max_iter=1)
                alone.append(timed(torch, lambda: P.advance(W["dt"]))[0])
            laden.append(timed(torch, both)[0])
    torch.cuda.synchronize()
    p, q, a = ms(np, plain), ms(np, laden), ms(np, alone)
    emit({"case": "steps", "particles": P.n, "steps_each": steps, "plain_step_ms_median": float(np.median(p)),
          "plain_step_ms_std": float(p.std()), "laden_step_ms_median": float(np.median(q)),
          "added_ms_per_step": float(np.median(q) - np.median(p)), "advance_alone_ms_median": float(np.median(a)),
          "alive": int((P.status() == 0).sum())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR")
    ap.add_argument("--bench-runs", type=int, default=2)
    ap.add_argument("--only-bench", action="store_true", help="part (iv) alone")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "particle_bench measures on the GPU; there is no CPU path"
    from probe_bench import build
    from tracer_bench import seeds

    def emit(r):
        r["mesh_N"] = a.N
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    if a.bench_trees:
        from viscosity_bench import bench_trees

        emit({"case": "bench", **bench_trees(a.bench_trees, a.bench_runs)})
    if a.only_bench:
        return 0
    S, W, clk, mesh = build(a.N)
    for _ in range(a.warmup):
        clk["t"] += W["dt"]
        S.solve(W["dt"], W["nu"], max_iter=1)
    x = seeds(W, "random", a.particles, 0)
    case_advance(S, W, x, a.reps, emit)
    case_classification(S, W, x, a.reps, emit)
    case_steps(S, W, clk, x, a.steps, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
