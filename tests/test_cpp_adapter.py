"""The C++ host-side adapters (include/ebvo/adapters.hpp) compile against the C ABI alone, and on a
GPU produce exactly the oracle's results when driven like the reference drives its classes."""
import os
import subprocess

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, synth
from tests import oracle as orc
from tests.util import assert_bit_equal, assert_edges_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "adapter_demo.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "adapter_demo")


def build_demo():
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
           "-L", libdir, "-lebvo_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)


def test_adapter_builds_with_plain_gxx():
    """No HIP, OpenCV or Eigen headers are needed on the host side of the boundary."""
    build_demo()
    assert os.path.exists(EXE)


def test_boundary_bench_builds_with_plain_gxx(tmp_path):
    """tools/boundary_bench.cpp (bench.py's boundary_pairs_per_s: the stage-wise sequence through the adapters)."""
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "boundary_bench")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "boundary_bench.cpp"), "-o", exe, "-L", libdir, "-lebvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_adapter_matches_oracle(tmp_path):
    build_demo()
    h, w = 96, 160
    l, r = synth.stereo_pair("s2", h, w)
    (tmp_path / "l.raw").write_bytes(l.tobytes())
    (tmp_path / "r.raw").write_bytes(r.tobytes())
    out = tmp_path / "out.bin"
    subprocess.check_call([EXE, str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(h), str(w), str(out)])
    buf = out.read_bytes()
    nL, nR, tL, tR, npairs = np.frombuffer(buf, dtype=np.int32, count=5)
    off = 20
    L = np.frombuffer(buf, dtype=orc.EDGE_DTYPE, count=nL, offset=off); off += 32 * nL
    R = np.frombuffer(buf, dtype=orc.EDGE_DTYPE, count=nR, offset=off); off += 32 * nR
    rp = np.frombuffer(buf, dtype=np.int32, count=nL + 1, offset=off); off += 4 * (nL + 1)
    ci = np.frombuffer(buf, dtype=np.int32, count=npairs, offset=off); off += 4 * npairs
    sims = np.frombuffer(buf, dtype=np.float64, count=4 * npairs, offset=off).reshape(-1, 4); off += 32 * npairs
    keep = np.frombuffer(buf, dtype=np.uint8, count=npairs, offset=off); off += npairs
    self_sim = np.frombuffer(buf, dtype=np.float64, count=1, offset=off)[0]; off += 8
    alpha = np.frombuffer(buf, dtype=np.float64, count=npairs, offset=off); off += 8 * npairs
    score = np.frombuffer(buf, dtype=np.float64, count=npairs, offset=off); off += 8 * npairs
    xy = np.frombuffer(buf, dtype=np.float64, count=2 * npairs, offset=off).reshape(-1, 2); off += 16 * npairs
    valid = np.frombuffer(buf, dtype=np.uint8, count=npairs, offset=off); off += npairs
    bnb_cnt = np.frombuffer(buf, dtype=np.int32, count=nL, offset=off); off += 4 * nL
    bnb_order = np.frombuffer(buf, dtype=np.int32, count=npairs, offset=off); off += 4 * npairs
    shifted = np.frombuffer(buf, dtype=orc.EDGE_DTYPE, count=npairs, offset=off); off += 32 * npairs
    cl_cnt = np.frombuffer(buf, dtype=np.int32, count=nL, offset=off); off += 4 * nL
    cl_of = np.frombuffer(buf, dtype=np.int32, count=npairs, offset=off); off += 4 * npairs
    best_cnt = np.frombuffer(buf, dtype=np.int32, count=nL, offset=off); off += 4 * nL
    fh = np.frombuffer(buf, dtype=np.int32, count=7, offset=off); off += 28
    nf = int(fh[5])
    f_left = np.frombuffer(buf, dtype=np.int32, count=nf, offset=off); off += 4 * nf
    f_right = np.frombuffer(buf, dtype=orc.EDGE_DTYPE, count=nf, offset=off); off += 32 * nf
    f_score = np.frombuffer(buf, dtype=np.float64, count=nf, offset=off); off += 8 * nf
    f_rows = np.frombuffer(buf, dtype=np.float64, count=16 * nf, offset=off).reshape(-1, 16); off += 128 * nf
    th = np.frombuffer(buf, dtype=np.int64, count=4, offset=off); off += 32
    n_kf_t, n_tq = int(th[0]), int(th[3])
    t_rp = np.frombuffer(buf, dtype=np.int32, count=n_kf_t + 1, offset=off); off += 4 * (n_kf_t + 1)
    t_cf = np.frombuffer(buf, dtype=np.int32, count=n_tq, offset=off); off += 4 * n_tq
    t_left = np.frombuffer(buf, dtype=orc.EDGE_DTYPE, count=n_tq, offset=off); off += 32 * n_tq
    t_right = np.frombuffer(buf, dtype=orc.EDGE_DTYPE, count=n_tq, offset=off); off += 32 * n_tq
    t_valid = np.frombuffer(buf, dtype=np.uint8, count=n_tq, offset=off); off += n_tq
    assert off == len(buf)
    ol, orr = orc.toed(l), orc.toed(r)
    assert (tL, tR) == (ol["n_total"], orr["n_total"])
    assert_edges_equal(L, ol["edges"])
    assert_edges_equal(R, orr["edges"])
    f, t = 718.856, 0.54
    F = np.array([0, 0, 0, 0, 0, -t / f, 0, t / f, 0], dtype=np.float64)
    lines = orc.epipolar_lines(F, ol["edges"])
    orp, oci = orc.epi_candidates(ol["edges"], orr["edges"], lines)
    assert_bit_equal(rp, orp)
    assert_bit_equal(ci, oci)
    osims, _, okeep, olp = orc.ncc_pairs(l, r, ol["edges"], orr["edges"][oci], orp)
    assert_bit_equal(sims, osims)
    assert_bit_equal(keep, okeep)
    assert self_sim == orc.patch_similarity(olp[0, 0], olp[0, 0])
    cand_xy = np.stack([orr["edges"]["x"][oci], orr["edges"]["y"][oci]], 1)
    ref = orc.gn_refine_stereo(l, r, ol["edges"], lines, orp, cand_xy)
    assert_bit_equal(alpha, ref["alpha"])
    assert_bit_equal(score, ref["score"])
    assert_bit_equal(xy, ref["refined_xy"])
    assert_bit_equal(valid, ref["validity"])
    # stage glue through the adapters
    obest = orc.ncc_pairs(l, r, ol["edges"], orr["edges"][oci], orp)[1]
    oc, oo = orc.bnb_test(orp, obest, 0.9, True)
    assert_bit_equal(bnb_cnt, oc, "bnb count")
    assert_bit_equal(bnb_order, oo, "bnb order")
    osh = orc.epipolar_shift(orr["edges"][oci], lines, orp)
    assert_edges_equal(shifted, osh)
    occ, _, ocof = orc.cluster_rows(osh, orp, False, True)
    assert_bit_equal(cl_cnt, occ, "cluster count")
    assert_bit_equal(cl_of, ocof, "cluster_of")
    assert_bit_equal(best_cnt, (np.diff(orp) > 0).astype(np.int32))
    # the output file of the reference's writer: header + 16 numbers per kept match at 6 significant digits
    kept = okeep.astype(bool)
    rows = np.repeat(np.arange(len(ol["edges"])), np.diff(orp))[kept]
    K = [f, 0, 607.1928, 0, f, 185.2157, 0, 0, 1]
    fin = orc.finalize_pairs(K, K, np.eye(3), [t, 0, 0], ol["edges"][rows], orr["edges"][oci[kept]])
    text = (tmp_path / "out.bin.txt").read_text().splitlines()
    assert text[0] == ("left_edge_location, left_edge_orientation, right_edge_location, right_edge_orientation, "
                       "left_edge_3D_point, left_edge_tangent")
    assert len(text) == 1 + len(fin)
    for line, row in zip(text[1:], fin):
        assert line == " ".join("%g" % v for v in row)          # std::ostream default == printf %g
    # StereoMatcherHIP::stereo_edge_pairs = get_Stereo_Edge_Pairs in one pass: against the chain of oracle functions
    from tests import oracle_chain
    stage1 = dict(l=l, r=r, F=F, left=ol["edges"], right=orr["edges"], row_ptr=orp, col_idx=oci, sims=osims, best=obest,
                  keep=okeep)
    ch = oracle_chain.stereo_edge_pairs(l, r, F, (K, K, np.eye(3).ravel(), [t, 0, 0]), stage1=stage1,
                                        cluster_args=(True, False), sift=True)
    want = ch["counts"]
    assert dict(n_sift=int(fh[0]), n_ncc=int(fh[1]), n_bnb=int(fh[2]), n_clusters=int(fh[3]), n_ncc2=int(fh[4]),
                n_final=int(fh[5])) == want and int(fh[6]) == len(oci) and nf > 100
    assert_bit_equal(f_left, ch["left_index"], "left_index")
    assert_edges_equal(f_right, ch["right"], "right centre")
    assert_bit_equal(f_score, ch["score"], "score")
    assert_bit_equal(f_rows, ch["rows"], "rows")

    # TemporalMatcherHIP: keyframe = this frame, next frame = the scene moved by 2 px -- against the Python binding of the same
    # entry points (which tests/test_gpu_temporal.py checks against the oracle-side chain)
    from edge_based_visual_odometry_amd.api import Context
    calib = (K, K, np.eye(3).ravel(), [t, 0, 0])
    with Context(h, w) as c:
        c.stereo_upload(l, r)
        c.stereo_run(c.default_params(F))
        c.stereo_finalize(calib, use_sift=True)
        c.temporal_set_keyframe()
        c.stereo_upload(np.roll(l, 2, axis=1), np.roll(r, 2, axis=1))
        c.stereo_run(c.default_params(F))
        c.stereo_finalize(calib, use_sift=True)
        counts, q = c.temporal_match(stages=1)
    assert (n_kf_t, int(th[1]), int(th[2]), n_tq) == (counts["n_kf"], counts["n_kept"], counts["n_bnb_sift"], counts["n_final"])
    assert n_tq > 50
    assert_bit_equal(t_rp, q["final"]["row_ptr"], "temporal row_ptr")
    assert_bit_equal(t_cf, q["final"]["cf_index"], "temporal cf_index")
    assert_edges_equal(t_left, q["final"]["left"], "temporal left centres")
    assert_edges_equal(t_right, q["final"]["right"], "temporal right centres")
    assert_bit_equal(t_valid, q["final"]["valid"], "temporal validity")


# ---- the input side: ebvo::undistort, ebvo::sift_descriptors, ebvo::sift_min_distances (tests/cpp/input_demo.cpp) ----------------
INPUT_SRC = os.path.join(ROOT, "tests", "cpp", "input_demo.cpp")
INPUT_EXE = os.path.join(ROOT, "tests", "cpp", "input_demo")


def build_input_demo():
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), INPUT_SRC,
                           "-o", INPUT_EXE, "-L", libdir, "-lebvo_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])


def test_input_demo_builds_with_plain_gxx():
    build_input_demo()
    assert os.path.exists(INPUT_EXE)


@pytest.mark.gpu
def test_input_adapters_match_oracle(tmp_path):
    """cv::undistort over the border (undistort_cases: pincushion), descriptors that saturate and vanish (sift_cases: step32)
    and their distances over a small CSR with empty rows, through the C++ adapters: the raw results against the oracle"""
    from tests import sift_cases as sc
    from tests import undistort_cases as uc
    build_input_demo()
    (h, w), K, dist = uc.CASES["pincushion"]
    img = uc.image("pincushion")
    simg, e = sc.case("step32")
    n = len(e)
    lens = np.array([0, 3, 0, 1] + [2] * (n - 6) + [0, 0])        # leading, interior and trailing empty rows
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cand = ((np.repeat(np.arange(n), lens) * 7 + np.arange(int(lens.sum()))) % n).astype(np.int32)
    blob = b"".join([np.array([h, w, len(dist)], dtype=np.int32).tobytes(), np.array(K, dtype=np.float64).tobytes(),
                     np.array(dist, dtype=np.float64).tobytes(), img.tobytes(),
                     np.array([simg.shape[0], simg.shape[1], n], dtype=np.int32).tobytes(), simg.tobytes(),
                     np.ascontiguousarray(e, dtype=orc.EDGE_DTYPE).tobytes(), np.array([len(cand)], dtype=np.int32).tobytes(),
                     row_ptr.tobytes(), cand.tobytes()])
    (tmp_path / "in.bin").write_bytes(blob)
    out = tmp_path / "out.bin"
    subprocess.check_call([INPUT_EXE, str(tmp_path / "in.bin"), str(out)])
    buf = out.read_bytes()
    assert len(buf) == h * w + 4 * 256 * n + 8 * len(cand)
    und = np.frombuffer(buf, dtype=np.uint8, count=h * w).reshape(h, w)
    desc = np.frombuffer(buf, dtype=np.float32, count=256 * n, offset=h * w).reshape(n, 2, 128)
    d = np.frombuffer(buf, dtype=np.float64, count=len(cand), offset=h * w + 1024 * n)
    assert (und == orc.undistort(img, K, dist)).all()
    ref = sc.oracle_descriptors("step32")
    assert_bit_equal(desc, ref, "descriptors")
    assert (desc == 255).any() and (~desc.any(axis=2)).any()
    assert_bit_equal(d, orc.sift_min_distances(ref, ref[cand], row_ptr), "min distances")
