"""The inputs of tests/test_gpu_temporal_edges.py meet the conditions that file relies on -- recomputed on the oracle alone
(no device): mate counts on both sides of the temporal kernels' work units, cell counts around cell_scan_kernel's 256
threads, crowded cells, the parameters that empty the chain in its middle, keyframe mates outside a smaller frame's grid."""
import numpy as np

from tests import temporal_cases as tc


def test_input_conditions():
    got = {name: tc.conditions(kf, cf, cell) for name, (kf, cf, cell, _) in tc.UNIT_CASES.items()}
    assert got == tc.EXPECTED
    n_kf = {c["n_kf"] for c in got.values()}
    n_cf = {c["n_cf"] for c in got.values()}
    # 16 mates per block and 4 per wave in temporal_candidates; 16 lanes per mate / quad in patches and ncc_quads_indexed
    assert {0, 1, 15} <= {n % 16 for n in n_kf} and {0, 1, 2, 3} <= {n % 4 for n in n_kf}
    assert {0, 1, 15} <= {n % 16 for n in n_cf}
    assert any(0 < n < 4 for n in n_kf) and min(n_kf) == 1 and any(0 < n < 16 for n in n_cf) and min(n_cf) == 1
    assert any(0 < c["n_candidates"] < 16 for c in got.values()) and max(c["n_candidates"] for c in got.values()) > 131072
    # cell_scan_kernel: fewer cells than threads, one each, more than one each with idle threads at the end
    cells = {c["n_cells"] for c in got.values()}
    assert min(cells) < 256 and 256 in cells and any(n > 256 and n % 256 for n in cells)
    # cell_sort_kernel's 64-lane stride: a cell of exactly 64 or 65 mates and a cell of more
    crowded = got["cells-104-crowded"]
    assert crowded["cells_64_65"] > 0 and crowded["max_cell"] > 65
    pop, _ = tc.cell_populations("cf2", 30)
    assert 64 in pop and 65 in pop


def test_empty_middles_are_the_intended_exits():
    levels, below, _ = tc.sift_levels("kf", "cf2")
    assert levels[0] > 0 and list(below[:3]) == [0, 1, 2]
    c = tc.reference("kf", "cf2", None, True, ncc_thr=2.0)["counts"]
    assert c["n_candidates"] > 0 and c["n_kept"] == 0 and c["n_final"] == 0
    c = tc.reference("kf", "cf2", None, True, sift_thr=float(levels[0]))["counts"]
    assert c["n_kept"] > 0 and c["n_sift"] == 0 and c["n_final"] == 0
    c = tc.reference("kf", "cf2", None, True, orient_thr_deg=0.0)["counts"]
    assert c["n_kf"] > 0 and c["n_cf"] > 0 and c["n_candidates"] == 0
    for n in (1, 2):
        c = tc.reference("kf", "cf2", None, True, sift_thr=float(levels[n]))["counts"]
        assert c["n_sift"] == n == c["n_final"]


def test_keyframe_mates_outside_a_smaller_grid():
    out, clipped = tc.rows_outside_grid("kf", "small2")
    rows = np.diff(tc.reference("kf", "small2", None, False)["row_ptr"])
    assert len(out) > 1000 and len(clipped) > 1000 and set(clipped) <= set(out)
    assert rows[clipped].sum() == 0 and rows[out].sum() > 0
    out, _ = tc.rows_outside_grid("small0", "cf2")
    assert len(out) == 0
