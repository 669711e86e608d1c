"""The Lagrangian average of the dynamic Smagorinsky model at the bench size (Taylor-Green 128^3, P2-P1): ONE solver in one
process, the protocol of tools/dynamic_bench.py (HIP events, 3 untimed and ``--reps`` timed launches per variant, the
variants alternating inside the timed loop, medians).

    python tools/lagrangian_bench.py [-N 128] [--warmup 3] [--reps 20] [--out FILE]
                                     [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, ``ox_dynamic_lagrangian`` at the bench's own CFL and at a velocity scaled so that the longest path is 3 cell widths
per update, beside ``ox_dynamic_vertices``, ``ox_patch_filter_vertices`` (k = 2) and ``ox_tracer_advance`` (Euler, one
substep, hint on) on the same points: one particle per mesh vertex.  Reported with each: the share of vertices whose
departure point lies in the hint cell, and the bytes of the hint path -- streamed (what a lane reads and writes of its own
row) and gathered (the hint cell's geometry, its vertex classes and their old fields); a vertex off the hint adds its
bin's list walk, 4 + 8 (gdim + gdim^2) bytes per entry.
Part 2, ``viscosity_assemble`` with the lagrangian, local and global models bound to the same solver.
Part 3 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees,
alternating: the default step makes no new call and must not change."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from viscosity_bench import HBM_PEAK, bench_trees, build, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per variant")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR")
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    import ctypes as C

    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib

    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    S, W, clk = build(a.N, ox.Smagorinsky())
    dt, nu = W["dt"], W["nu"]
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    models = {"lagrangian": ox.DynamicSmagorinsky(average="lagrangian"), "local": ox.DynamicSmagorinsky(average="local"),
              "global": ox.DynamicSmagorinsky()}
    for m in models.values():
        m.bind(S)
        for _ in range(2):  # (the Lagrangian model: the second evaluation is the first with a back-trace)
            m.evaluate(S, S._nut, nu, **({"dt": dt} if m.needs_dt else {}))
    torch.cuda.synchronize()

    lib, st = _lib.load(), _lib.current_stream()
    lag = models["lagrangian"]
    p = lag._patches
    nc, nv, d, nr, nm = p.n_cells, p.n_vertices, p.gdim, lag._nr, lag._nm
    vol = C.c_void_p(lag._rec.data_ptr() + 8 * (nr - 1))
    u_own = lag._mom[:, :d].contiguous()
    speed = torch.sqrt((u_own * u_own).sum(dim=1))
    width = float(W["box"][1][0] - W["box"][0][0]) / a.N
    scale3 = 3.0 * width / (dt * float(speed.max()))
    u_fast = (u_own * scale3).contiguous()
    f_old, f_new = lag._f[lag._cur], lag._f[1 - lag._cur]

    def hint_share(u):
        xp = lag._xv - dt * u
        lam = lag._tree.bary(xp, lag._hint).min(dim=1).values
        # (the second: the share that a hint test with the locator's tolerance would resolve -- points ON a facet of the hint)
        return float((lam >= 0.0).double().mean()), float((lam >= -lag._loc_tol).double().mean())

    def lagrangian(u):
        args = lag.lagrangian_args(dt, False, u, d, lag._src, f_old, f_new, lag._cs2v, lag._status)
        _lib.check(lib.ox_dynamic_lagrangian(C.byref(args), st), "ox_dynamic_lagrangian")

    tr = ox.Tracers(S, lag._xv, scheme="euler", substeps=1, sort_every=0)
    state = [t.clone() for t in (tr._x, tr._cell, tr._status, tr._age, tr._path, tr._t_exit)]

    def tracer():
        tr.advance(dt)

    def tracer_reset():
        for t, s in zip((tr._x, tr._cell, tr._status, tr._age, tr._path, tr._t_exit), state):
            t.copy_(s)

    variants = {
        "lagrangian_bench_cfl": lambda: lagrangian(u_own),
        "lagrangian_3_cells": lambda: lagrangian(u_fast),
        "dynamic_vertices": lambda: _lib.check(lib.ox_dynamic_vertices(d, nv, _lib.ptr(p.ptr), _lib.ptr(p.idx), nc,
                                                                       _lib.ptr(lag._rec), _lib.ptr(lag._mom), st), "vertices"),
        "filter_vertices_k2": lambda: _lib.check(lib.ox_patch_filter_vertices(2, nv, _lib.ptr(p.ptr), _lib.ptr(p.idx), nc,
                                                                              p.n_idx, _lib.ptr(lag._lm), vol, nr,
                                                                              _lib.ptr(lag._src), st), "filter_vertices"),
        "tracer_advance_euler": tracer,
    }
    ev = {k: [] for k in variants}
    for _ in range(a.reps + 3):
        for k, fn in variants.items():
            if k == "tracer_advance_euler":
                tracer_reset()
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    status_own = None
    kern = {}
    streamed = nv * (2 * d * 8 + 8 + 16 + 8 + 16 + 16 + 8 + 4)
    gathered = nv * ((d + d * d) * 8 + 8 + (d + 1) * 4 + (d + 1) * 16)
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4)}
    for k, u in (("lagrangian_bench_cfl", u_own), ("lagrangian_3_cells", u_fast)):
        lagrangian(u)
        torch.cuda.synchronize()
        stt = torch.bincount(lag._status.to(torch.int64), minlength=3).tolist()
        if status_own is None:
            status_own = stt
        ms = kern[k]["ms"]
        hs = hint_share(u)
        kern[k].update(hint_share=round(hs[0], 4), hint_share_within_tol=round(hs[1], 4), status_counts=stt, streamed_bytes=streamed,
                       gather_bytes_hint_path=gathered,
                       fraction_of_hbm_peak_hint_path=round((streamed + gathered) / (ms * 1e-3) / HBM_PEAK, 3),
                       max_path_in_cell_widths=round(float((torch.sqrt((u * u).sum(dim=1))).max()) * dt / width, 3))
    kern["dynamic_vertices"].update(streamed_bytes=(nv + 1) * 4 + p.n_idx * 4 + nv * nm * 8, gather_bytes=p.n_idx * nr * 8)
    kern["filter_vertices_k2"].update(streamed_bytes=(nv + 1) * 4 + p.n_idx * 4 + nv * 16, gather_bytes=p.n_idx * 24)
    kern["tracer_advance_euler"].update(points=tr.n, alive=int((state[2] == 0).sum()))
    info = lag._tree.info() if hasattr(lag._tree, "info") else {}

    # ---- part 2: viscosity_assemble of the three averages, alternating ---------------------------------------------------
    rec = {k: [] for k in models}
    for _ in range(a.reps + 3):
        for k, m in models.items():
            kw = {"dt": dt} if m.needs_dt else {}
            rec[k].append(timed(torch, lambda m=m, kw=kw: m.evaluate(S, S._nut, nu, **kw)))
    torch.cuda.synchronize()
    assemble = {k: round(statistics.median(x.elapsed_time(y) for x, y in v[3:]), 4) for k, v in rec.items()}
    cs2 = lag.coefficient_cells(S)
    out = {"N": a.N, "cells": nc, "vertices": nv, "dt": dt, "nu": nu, "cell_width": width,
           "locator": {k: (v if isinstance(v, (int, float, str)) else list(v)) for k, v in dict(info).items()},
           "kernel": kern, "viscosity_assemble_ms": assemble,
           "cs2_lagrangian_min_mean_max": [float(cs2.min()), float(cs2.mean()), float(cs2.max())]}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
