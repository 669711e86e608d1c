"""GPU: whole IPCS steps of the channel of tests/channel_problem.py -- time-dependent inlet, no-slip walls and a pressure
outlet located through mesh tags, with and without the rotational pressure update -- on the rank THREADS of one process
(tests/helpers.py ``run_rank_threads``, as tests/test_gpu_threads_rehearsal.py), against the serial run.

What meets here for the first time with ``comm.size > 1``: the outlet term on a ``b_first`` with ghost rows, the pressure
solve on an operator with identity rows and zeroed (ghost) columns and without the two mean removals, the rotational
update's mass product, divergence and ``Projector`` solve with their exchanges, and the copy of its result into ``ps``
over owned and ghost entries.  Ranks without an outlet facet pass through the same collective points as ranks with one."""
import numpy as np
import pytest
import torch

from tests import channel_problem as CP

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ranks,kind,N,low_memory,rotational,h", [
    (8, "box", 4, True, False, "float"),
    (8, "box", 4, True, True, "float"),
    (8, "box", 4, False, True, "callable"),
    (4, "rect", 8, True, True, "float"),
    (8, "delaunay", 4, True, True, "float"),
])
def test_rank_threads_step_the_channel_like_the_serial_run(hip, ranks, kind, N, low_memory, rotational, h):
    """Two ``solve(dt, nu, max_iter=1)`` steps, P2-P1; every rank's ``U1`` and ``P``, owned AND ghost entries, against the
    serial run through the dof coordinates.  Bounds: the rehearsal's ``du < 1e-8``, ``dp < 1e-7``, relative to
    ``max(1, max|field|)`` of the serial run (both runs are Krylov solves to rtol 1e-11).  Measured on an MI355X: ``du`` and
    ``dp`` at most 1.4e-14 on the lattice meshes and 6.8e-12 / 5.6e-12 on the Delaunay mesh, with ``max|u|`` 6 to 24 and
    ``max|p|`` 11 to 37 (``-s`` prints them): the outlet term ``h n_i dv/dx_i`` scales with ``h`` over the mesh size, so
    the fields of this set-up are not of order one."""
    from tests.helpers import run_rank_threads

    def run(comm):
        prob = CP.build(kind, N, comm, (2, 1), h, low_memory, rotational)
        diffs = CP.run_steps(prob, 2)
        torch.cuda.synchronize()
        return prob, diffs

    G, gdiffs = run(None)
    Vg, Qg = G.S._Vi[0][0], G.S._Q
    tu, tq = CP.lookup(Vg.x.cpu().numpy()), CP.lookup(Qg.x.cpu().numpy())
    ug, pg = G.S._U1.dev().cpu().numpy(), G.S._P.dev().cpu().numpy()[:, 0]
    su, sp = max(1.0, float(np.abs(ug).max())), max(1.0, float(np.abs(pg).max()))
    assert np.isfinite(ug).all() and np.isfinite(pg).all() and np.abs(pg).max() > 1.0

    def rank_job(comm):
        prob, diffs = run(comm)
        S = prob.S
        Vi, Q = S._Vi[0][0], S._Q
        assert Vi.dist is not None and Q.dist is not None and comm.active == {2: "host", 1: "host"}, comm.active
        iu, iq = CP.to_serial(tu, Vi.x.cpu().numpy()), CP.to_serial(tq, Q.x.cpu().numpy())
        ul, pl = S._U1.dev().cpu().numpy(), S._P.dev().cpu().numpy()[:, 0]
        return {"du": float(np.abs(ul - ug[iu]).max()) / su, "dp": float(np.abs(pl - pg[iq]).max()) / sp, "diff": diffs[-1],
                "owned": (int(Vi.n_owned), int(Q.n_owned)), "ghosts": (int(Vi.n_local - Vi.n_owned), int(Q.n_local - Q.n_owned)),
                "facets": int(prob.bcp._n_facets), "its": {k: [int(i) for i in v] for k, v in S.iteration_counts().items()}}

    res, world = run_rank_threads(ranks, rank_job)
    print(f"\n{kind} N={N} on {ranks} rank threads, low_memory={low_memory}, rotational={rotational}, h {h}: "
          f"du = {max(r['du'] for r in res):.3e}, dp = {max(r['dp'] for r in res):.3e} (relative to {su:.3f}, {sp:.3f}); "
          f"outlet facets per rank {[r['facets'] for r in res]}; iterations {res[0]['its']}; "
          f"all-reduces {world.allreduces[0]}, exchanges {world.exchanges}")
    assert sum(r["owned"][0] for r in res) == Vg.num_dofs and sum(r["owned"][1] for r in res) == Qg.num_dofs
    assert min(r["ghosts"][1] for r in res) > 0
    assert min(r["facets"] for r in res) == 0 < max(r["facets"] for r in res)  # ranks with and without an outlet
    for r in res:
        assert r["du"] < 1e-8 and r["dp"] < 1e-7, res  # owned AND ghost entries agree with the serial run
        assert abs(r["diff"] - gdiffs[-1]) < 1e-8 * max(1.0, abs(gdiffs[-1]))
        assert r["its"] == res[0]["its"]  # the lock-step's decisions are all-reduced: the same on every rank
    # every rank, with an outlet or without, went through the same number of collective points
    assert len(set(world.allreduces)) == 1 and world.allreduces[0] > 0 and min(world.exchanges) > 0
