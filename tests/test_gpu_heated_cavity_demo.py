"""GPU: demo/heated_cavity_hip.py runs and prints its table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_demo_prints_the_nusselt_table(hip, capsys, tmp_path):
    """-N 8, the default 60 steps: the table with both wall Nusselt numbers and the velocity maxima beside the benchmark's
    values, within 1 % and 2 % of them at this resolution; --out writes the walls' .vtu and .npz."""
    from demo.heated_cavity_hip import main

    res = main(["-N", "8", "--out", str(tmp_path / "walls.vtu")])
    out = capsys.readouterr().out
    for word in ("Nusselt, hot wall", "Nusselt, cold wall", "max |u|", "max |v|", "benchmark", "1.118", "3.649", "3.697"):
        assert word in out, (word, out)
    assert abs(res["nu_hot"] - 1.118) < 0.01 * 1.118 and abs(res["nu_cold"] - 1.118) < 0.01 * 1.118
    assert abs(res["umax"] - 3.649) < 0.02 * 3.649 and abs(res["vmax"] - 3.697) < 0.02 * 3.697
    assert res["history"].shape == (60, 2) and np.isfinite(res["history"]).all()
    assert (tmp_path / "walls.vtu").exists() and (tmp_path / "walls.npz").exists()
