#!/usr/bin/env python3
"""Profiles of the periodic channel of demo/periodic_channel_hip.py at its steady Poiseuille state, HIP path.

The channel is driven from rest by the body force (G, 0[, 0]) until the start-up transient has died out, then
``oasisx_amd.ProfileStatistics`` averages the velocity over the slabs between the mesh planes of the wall-normal axis y
(the homogeneous directions x [and z] and time) for ``--samples`` further steps.  The steady state is the parabola
U(y) = G (1 - y^2) / (2 nu), which P2 holds exactly: the profile of u_x is printed beside the exact slab means of the
parabola, G / (2 nu) (1 - (y1^3 - y0^3) / (3 (y1 - y0))), and the largest Reynolds stress, which is zero up to the
tolerance of the solves, beside the slab variance of u_x, (the spatial variance of the parabola inside a slab, which a slab
average cannot tell from a fluctuation: it falls as h^2).

    python demo/channel_profiles_hip.py [-N 8] [--dim 2] [--steps 200] [--samples 10] [--dt 0.1] [--nu 0.5] [-G 1.0]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from periodic_channel_hip import build_channel  # noqa: E402

TOLERANCE = 1e-7  # of the profile against the parabola, relative to its peak: the transient left after --steps, the solves


def parabola_slab_moments(edges, nu, G):
    """Exact slab mean and slab variance of U(y) = G (1 - y^2) / (2 nu) between consecutive ``edges``."""
    y0, y1 = edges[:-1], edges[1:]
    h = y1 - y0
    m2 = (y1 ** 3 - y0 ** 3) / (3.0 * h)
    m4 = (y1 ** 5 - y0 ** 5) / (5.0 * h)
    a = G / (2.0 * nu)
    return a * (1.0 - m2), a * a * (m4 - m2 * m2)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=8, help="cells across the channel")
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--steps", type=int, default=200, help="steps before the averaging starts")
    ap.add_argument("--samples", type=int, default=10, help="steps that are averaged")
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--nu", type=float, default=0.5)
    ap.add_argument("-G", type=float, default=1.0, help="body force along x")
    a = ap.parse_args(argv)
    import oasisx_amd as ox

    mesh, S = build_channel(a.N, a.dim, a.nu, a.G)
    P = ox.ProfileStatistics(S, axis=1, fields=("u", "p"))
    print(f"periodic channel, {a.dim}-D: {mesh.num_cells} cells in {P.n_bins} slabs along y, {P.n_chunks} chunks")
    for _ in range(a.steps):
        S.solve(a.dt, a.nu, max_iter=1)
    for _ in range(a.samples):
        S.solve(a.dt, a.nu, max_iter=1)
        P.sample(a.dt)
    y = P.coordinates()
    mean = P.mean("u").cpu().numpy()
    cov = P.covariance("u").cpu().numpy()
    want, var = parabola_slab_moments(P.edges, a.nu, a.G)
    peak = a.G / (2.0 * a.nu)
    print(f"{'y':>10} {'<u_x>':>16} {'parabola':>16} {'difference':>12} {'<u_x u_x>':>14} {'slab variance':>14}")
    for k in range(P.n_bins):
        print(f"{y[k]:>10.5f} {mean[k, 0]:>16.12f} {want[k]:>16.12f} {mean[k, 0] - want[k]:>12.3e} {cov[k, 0]:>14.6e} {var[k]:>14.6e}")
    err = float(np.abs(mean[:, 0] - want).max()) / peak
    cross = np.abs(mean[:, 1:]).max() / peak
    other = cov.copy()
    other[:, 0] -= var  # what is left of <u_x' u_x'> beside the parabola's own variance inside the slab
    stress = float(np.abs(other).max()) / peak ** 2
    print(f"max |<u_x> - parabola| / peak = {err:.3e} (tolerance {TOLERANCE:.1e})")
    print(f"max |<u_y>|[, |<u_z>|] / peak = {cross:.3e}")
    print(f"largest Reynolds stress beside the slab variance of the parabola / peak^2 = {stress:.3e} (tolerance {TOLERANCE:.1e})")
    print(f"total weight {P.total_weight:.6g} over {P.n_samples} samples, volume {float(P.volume().sum()):.12g}")
    return dict(error=err, stress=stress, tolerance=TOLERANCE, y=y, mean=mean, cov=cov)


if __name__ == "__main__":
    r = main()
    sys.exit(0 if r["error"] <= r["tolerance"] and r["stress"] <= r["tolerance"] else 1)
