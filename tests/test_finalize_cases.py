"""The inputs of tests/test_gpu_finalize_edges.py meet the conditions that file relies on -- recomputed on the oracle alone
(no device): kept rows of exactly 64 and of more into the Best-Nearly-Best test and into the clustering, rows of more than
256 with equal scores, more long rows than one block can queue, the four empty or untouched stages, pair runs of one and
two candidates, edge counts around a block of 256, and enough focused rows for the comparison of the intermediate lists."""
import time

from tests import finalize_cases as fc


def test_input_conditions():
    got = {name: fc.conditions(name) for name in fc.EXPECTED if name != "tiny"}
    assert got == {k: v for k, v in fc.EXPECTED.items() if k != "tiny"}
    # no small default pair reaches bnb_kernel's wave path with more than a handful of rows, none reaches 64
    assert all(got[n]["longest"] < 64 and got[n]["rows_17_256"] < 32 for n in ("default", "default120", "tiny48"))
    assert {got[n]["n_left"] % 256 for n in ("nl0", "nl1", "nl255")} == {0, 1, 255}


def test_long64_rows_enter_both_kernels():
    c = fc.conditions("long64")
    # bnb_kernel: rows of 17 .. 256 take the wave path; one block (cap 1) queues 512 of them and sorts the rest serially
    assert c["n_pairs"] == c["n_matches"] and c["rows_64"] > 0 and c["rows_over_64"] > 0 and c["rows_17_256"] > 512
    assert fc.rows_with_equal_scores("long64", 16) == []       # ... and the parallel ranking, not lane 0's sort, orders them
    # cluster_kernel: bnb_ratio = 0 carries rows of exactly 64 (the full presence mask) and of more (cluster_row_serial) on
    rows = fc.chain("long64", bnb_ratio=0.0)["stage_rows"]
    assert (rows["NCC"] == fc.kept_rows("long64")).all()
    for stage in ("BNB_NCC", "REFINE"):
        assert (rows[stage] == 64).any() and (rows[stage] > 64).any(), stage
    assert rows["CLUSTER"].max() < 64 and rows["CLUSTER"].sum() < rows["REFINE"].sum()
    # the default ratio prunes every row below 64 before the clustering: only the Best-Nearly-Best test sees the long ones
    assert fc.chain("long64")["stage_rows"]["BNB_NCC"].max() < 64
    counts = [fc.chain("long64", **kw)["counts"] for kw in ({}, dict(bnb_ratio=0.0))]
    assert all(c["n_final"] > 3000 for c in counts) and counts[0] != counts[1]


def test_long256_rows_hold_equal_scores_and_the_oracle_is_quick():
    c = fc.conditions("long256")
    assert c["rows_over_256"] > 0 and c["longest"] > 256
    ties = fc.rows_with_equal_scores("long256", 256)
    assert len(ties) > 0
    t0 = time.perf_counter()
    counts = fc.chain("long256")["counts"]
    assert time.perf_counter() - t0 < fc.LONG256_ORACLE_SECONDS
    assert counts["n_ncc"] == c["n_pairs"] and counts["n_final"] > 100


def test_empty_stages_are_the_intended_ones():
    n_pairs = fc.EXPECTED["default"]["n_pairs"]
    pair, fin = fc.EMPTY["a-no-kept-match"]
    s = fc.stage1("default", **pair)
    assert len(s["col_idx"]) == n_pairs > 0 and int(s["keep"].sum()) == 0
    assert set(fc.chain("default", pair, **fin)["counts"].values()) == {0}
    pair, fin = fc.EMPTY["b-no-sift-survivor"]
    c = fc.chain("default", pair, **fin)["counts"]
    assert c["n_sift"] == 0 and set(c.values()) == {0}
    pair, fin = fc.EMPTY["c-no-second-ncc-survivor"]
    c = fc.chain("default", pair, **fin)["counts"]
    assert c["n_clusters"] > 0 and c["n_ncc2"] == 0 and c["n_final"] == 0
    pair, fin = fc.EMPTY["d-both-bnb-ratios-zero"]
    ch = fc.chain("default", pair, **fin)
    c, rows = ch["counts"], ch["stage_rows"]
    # nothing dropped by either test: the lists before and after them are the same length on every row
    assert c["n_bnb"] == c["n_ncc"] > 0 and (rows["NCC"] == rows["BNB_NCC"]).all() and (rows["BNB_NCC"] == rows["BNB_SIFT"]).all()
    assert c["n_final"] > 0 and c != fc.chain("default", sift=True)["counts"]


def test_tiny_thresholds_list_one_and_two_pairs():
    seen = []
    for thr, n_pairs in fc.tiny_thresholds():
        s = fc.stage1("default", epi_thr=thr)
        assert len(s["col_idx"]) == n_pairs, thr
        seen.append((n_pairs, fc.chain("default", dict(epi_thr=thr))["counts"]["n_final"]))
    assert seen == fc.EXPECTED["tiny"] and {n for n, _ in seen} == {0, 1, 2}


def test_intermediate_lists_have_focused_long_rows():
    for case, (name, fin, long_row) in fc.GT_CASES.items():
        foc = fc.gt(name)[1]["focused"].astype(bool)
        assert 2 * int(foc.sum()) >= len(foc), case
        rows = fc.chain(name, **fin)["stage_rows"]
        ev = fc.gt_stages(name, **fin)
        assert set(rows) == ({"NCC", "BNB_NCC", "REFINE", "CLUSTER", "NCC2", "BEST"} | ({"SIFT", "BNB_SIFT"} if fin.get("sift") else set()))
        for stage, sid in fc.STAGE_ID.items():
            if stage in rows:   # oracle_gt's own composition of the chain lists the same number of candidates on every focused row
                assert (ev[sid][0][foc, 0] == rows[stage][foc]).all(), (case, stage)
        if long_row:
            for stage in ("NCC", "BNB_NCC", "REFINE"):
                assert rows[stage][foc].max() > 64 and (rows[stage][foc] == 64).any(), (case, stage)
    # every stage of the chain without a kept match is an empty list on every row
    pair, _ = fc.EMPTY["a-no-kept-match"]
    ev = fc.gt_stages("default", pair=pair, sift=True)
    assert all(not ev[sid][0].any() for stage, sid in fc.STAGE_ID.items() if stage != "SIFT") and ev[fc.STAGE_ID["SIFT"]][0].any()
