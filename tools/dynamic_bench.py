"""The dynamic Smagorinsky procedure at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm start): ONE solver in
one process, built with ``viscosity_model=Smagorinsky()``; the dynamic models (global, slabs along axis 1, local) are
bound to the same solver and swapped in, so every variant runs on the same matrices, fields and memory.  HIP events,
medians, the variants alternating inside the timed loops.

    python tools/dynamic_bench.py [-N 128] [--steps 8] [--warmup 3] [--reps 20] [--out FILE]
                                  [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, every new launch, alternating, beside ``ox_cell_viscosity`` (Smagorinsky) and ``ox_profile_cells`` (the velocity
group of ``ProfileStatistics(axis=1)``).  Bytes per launch from the stored sizes: what is streamed (dof lists, geometry,
records written) counts once; a gathered table counts twice -- ``gather_bytes`` (what the lanes request) and
``unique_bytes`` (every table entry once: what has to come from HBM if the caches serve the re-reads).
Part 2, ``viscosity_assemble`` and whole steps with each model and ``update_every`` 1 and 4 against ``Smagorinsky()``.
Part 3 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees
(this commit, the parent commit), alternating: the default step makes no new call and must not change."""
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
    ap.add_argument("--steps", type=int, default=8, help="timed steps per variant")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel variant")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR")
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    import ctypes as C

    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd.viscosity import _cell_viscosity

    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    smag = ox.Smagorinsky()
    S, W, clk = build(a.N, smag)
    dt, nu = W["dt"], W["nu"]
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    models = {"global": ox.DynamicSmagorinsky(), "slabs": ox.DynamicSmagorinsky(axis=1),
              "local": ox.DynamicSmagorinsky(average="local")}
    for m in models.values():
        m.bind(S)
        m.evaluate(S, S._nut, nu)
    torch.cuda.synchronize()

    lib, st = _lib.load(), _lib.current_stream()
    Vi = S._Vi[0][0]
    g, sl, lo = models["global"], models["slabs"], models["local"]
    p = g._patches
    nc, nv, nd, gs = p.n_cells, p.n_vertices, int(Vi.cell_dofs.shape[1]), int(S._geom.shape[1])
    nr, nm, d = g._nr, g._nm, p.gdim
    n_dofs = int(Vi.n_local)
    vol = C.c_void_p(g._rec.data_ptr() + 8 * (nr - 1))
    ps = ox.ProfileStatistics(S, axis=1, fields=("u",))
    ps.sample(dt)
    pg = ps._groups[0]

    def bin_sums(m):
        pl = m._plan
        _lib.check(lib.ox_dynamic_bin_sums(nc, _lib.ptr(m._lm), vol, nr, _lib.ptr(pl["order"]), _lib.ptr(pl["chunks"]),
                                           pl["n_chunks"], _lib.ptr(m._partials), st), "ox_dynamic_bin_sums")

    def bin_coef(m):
        _lib.check(lib.ox_dynamic_bin_coefficients(m.n_bins, _lib.ptr(m._plan["bin_chunk_ptr"]), _lib.ptr(m._partials),
                                                   m.cs2_max, _lib.ptr(m._bins), st), "ox_dynamic_bin_coefficients")

    def cellcoef(m):
        if m.average == "local":
            _cell_viscosity(S, S._nut, cs2=_lib.ptr(m._cs2), cs2_stride=1, n_coef=nc)
        else:
            _cell_viscosity(S, S._nut, cs2=C.c_void_p(m._bins.data_ptr() + 24), cs2_stride=4, n_coef=m.n_bins,
                            cell_bin=_lib.ptr(m._cell_bin))

    F = lo._filter
    variants = {
        "eddy_viscosity": lambda: _cell_viscosity(S, S._nut, model=0, coefficient=0.1677),
        "profile_cells": lambda: ps._cells(pg, pg.sources, pg.mean),
        "dynamic_cells": lambda: _lib.check(lib.ox_dynamic_cells(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs),
                                                                 S._UAB.rptr(), _lib.ptr(g._rec), st), "cells"),
        "dynamic_vertices": lambda: _lib.check(lib.ox_dynamic_vertices(d, nv, _lib.ptr(p.ptr), _lib.ptr(p.idx), nc,
                                                                       _lib.ptr(g._rec), _lib.ptr(g._mom), st), "vertices"),
        "dynamic_products": lambda: _lib.check(lib.ox_dynamic_products(d, nc, _lib.ptr(p.cell_verts), nv, _lib.ptr(g._rec),
                                                                       _lib.ptr(g._mom), 2.0, _lib.ptr(g._lm), st), "products"),
        "bin_sums_global": lambda: bin_sums(g),
        "bin_sums_slabs": lambda: bin_sums(sl),
        "bin_coefficients_global": lambda: bin_coef(g),
        "bin_coefficients_slabs": lambda: bin_coef(sl),
        "filter_vertices_k2": lambda: _lib.check(lib.ox_patch_filter_vertices(2, nv, _lib.ptr(p.ptr), _lib.ptr(p.idx), nc,
                                                                              p.n_idx, _lib.ptr(g._lm), vol, nr,
                                                                              _lib.ptr(F._qv), st), "filter_vertices"),
        "filter_cells_k2": lambda: _lib.check(lib.ox_patch_filter_cells(2, d, nc, _lib.ptr(p.cell_verts), nv, _lib.ptr(F._qv),
                                                                        _lib.ptr(lo._lmf), st), "filter_cells"),
        "clip_local": lambda: _lib.check(lib.ox_dynamic_clip(nc, _lib.ptr(lo._lmf), lo.cs2_max, _lib.ptr(lo._cs2), st), "clip"),
        "cellcoef_bins": lambda: cellcoef(sl),
        "cellcoef_cells": lambda: cellcoef(lo),
    }
    cell_stream = nc * (nd * 4 + gs * 8)
    dof_gather, dof_unique = nc * nd * d * 8, n_dofs * d * 8
    nchs = sl._plan["n_chunks"]
    nbytes = {  # (streamed, gathered as requested, the gathered tables once)
        "eddy_viscosity": (cell_stream + nc * 8, dof_gather, dof_unique),
        "dynamic_cells": (cell_stream + nc * nr * 8, dof_gather, dof_unique),
        "dynamic_vertices": ((nv + 1) * 4 + p.n_idx * 4 + nv * nm * 8, p.n_idx * nr * 8, nc * nr * 8),
        "dynamic_products": (nc * ((d + 1) * 4 + 8 + 16), nc * (d + 1) * nm * 8, nv * nm * 8),
        "bin_sums_global": (nc * (4 + 16 + 8) + g._plan["n_chunks"] * 32, 0, 0),
        "bin_sums_slabs": (nc * (4 + 16 + 8) + nchs * 32, 0, 0),
        "filter_vertices_k2": ((nv + 1) * 4 + p.n_idx * 4 + nv * 16, p.n_idx * 24, nc * 24),
        "filter_cells_k2": (nc * ((d + 1) * 4 + 16), nc * (d + 1) * 16, nv * 16),
        "clip_local": (nc * 24, 0, 0),
        "cellcoef_bins": (cell_stream + nc * 12, dof_gather, dof_unique),
        "cellcoef_cells": (cell_stream + nc * 16, dof_gather, dof_unique),
    }
    ev = {k: [] for k in variants}
    for _ in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4)}
        if k in nbytes:
            s_, gth, uni = nbytes[k]
            kern[k].update(streamed_bytes=s_, gather_bytes=gth, unique_bytes=uni,
                           fraction_of_hbm_peak_unique=round((s_ + uni) / (ms * 1e-3) / HBM_PEAK, 3),
                           fraction_of_hbm_peak_requested=round((s_ + gth) / (ms * 1e-3) / HBM_PEAK, 3))
    count = torch.diff(p.ptr.to(torch.int64))
    patch = {"min": int(count.min()), "mean": round(float(count.double().mean()), 2), "max": int(count.max())}

    # ---- part 2: viscosity_assemble and whole steps, alternating ---------------------------------------------------------
    runs = [("smagorinsky", smag, 1)] + [(f"{k}_every{n}", m, n) for k, m in models.items() for n in (1, 4)]
    phase = []
    inner = S.viscosity_assemble

    def wrapped(*args):
        phase.append(timed(torch, lambda: inner(*args)))

    S.viscosity_assemble = wrapped
    rec = {k: {"step": [], "nut": []} for k, _, _ in runs}
    seen = {k: 0 for k, _, _ in runs}  # assemble_first calls of each variant (two variants share one model object)
    for i in range(a.steps + 1):
        for key, m, n in runs:
            S._viscosity_model = m
            if m is not smag:
                m.update_every, m.n_evaluations = n, seen[key]
            seen[key] += 1
            phase.clear()
            clk["t"] += dt
            e = timed(torch, lambda: S.solve(dt, nu, max_iter=1))
            torch.cuda.synchronize()
            if i == 0:
                continue
            rec[key]["step"].append(e[0].elapsed_time(e[1]))
            rec[key]["nut"].append(sum(x.elapsed_time(y) for x, y in phase))
    steps = {}
    for key, m, n in runs:
        v = rec[key]
        steps[key] = {"ms_per_step": round(statistics.median(v["step"]), 3),
                      "viscosity_assemble_ms_median": round(statistics.median(v["nut"]), 4),
                      "viscosity_assemble_ms_mean": round(statistics.fmean(v["nut"]), 4),
                      "viscosity_assemble_ms_all": [round(x, 4) for x in v["nut"]]}
    S._viscosity_model = models["slabs"]
    models["slabs"].update_every = 1
    models["slabs"].n_evaluations = 0
    S.assemble_first(dt, nu)
    cs2 = models["slabs"].bin_coefficients(clipped=False)
    nut = S.eddy_viscosity()
    out = {"N": a.N, "cells": nc, "vertices": nv, "dofs_u": n_dofs, "patch_cells": patch, "record_doubles": nr,
           "moment_doubles": nm, "chunks_global": g._plan["n_chunks"], "chunks_slabs": nchs, "bins_slabs": sl.n_bins,
           "nu": nu, "dt": dt, "kernel": kern, "steps": steps,
           "slab_cs2_min_max": [float(cs2.min()), float(cs2.max())],
           "nut_min_mean_max": [float(nut.min()), float(nut.mean()), float(nut.max())]}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
