"""The pose prior through the C++ adapters (include/ebvo/adapters.hpp: TemporalMatcherHIP::set_prior / clear_prior,
ebvo::predict_pose): tests/cpp/tprior_demo.cpp compiles against the C ABI alone, its predict_pose is the Python one, and on a
GPU set_prior + match returns the oracle's quads of the resident case of tests/test_gpu_tprior.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, api
from tests import oracle as orc
from tests import oracle_chain
from tests import tprior_cases as cases
from tests.util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_demo(tmp_path):
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "tprior_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "tprior_demo.cpp"), "-o", exe, "-L", libdir, "-lebvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_demo_builds_with_plain_gxx_and_predict_pose_is_the_python_one(tmp_path):
    exe = build_demo(tmp_path)
    lines = subprocess.check_output([exe], text=True).splitlines()
    rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    T1 = (rz, np.array([1.0, 0, 0]))
    T2 = (rz @ rz, np.array([0.0, 1, 2]))
    for line, (R, t) in zip(lines, (api.predict_pose(T2, T1), api.predict_pose(T2))):
        got = np.array([float(v) for v in line.split()[1:]])
        assert_bit_equal(got[:9].reshape(3, 3) + 0.0, R + 0.0, line.split()[0] + " R")      # (+ 0.0: -0 and 0 are one pose)
        assert_bit_equal(got[9:] + 0.0, t + 0.0, line.split()[0] + " t")
    R, t = api.predict_pose(T2, T1)
    assert (R == [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]).all() and (t == [-1, 0, 4]).all()    # D T2 with D = (Rz 90, (0, 0, 2))


@pytest.mark.gpu
def test_adapter_returns_the_oracles_quads(tmp_path):
    exe = build_demo(tmp_path)
    name = "short-r8"
    px, radius, use_orientation = cases.RESIDENT[name]
    R, t = cases.prior_pose(px)
    cal = api.Context._calib(cases.CALIB)
    head = b"".join([np.array([cases.H, cases.W], dtype=np.int32).tobytes(), np.asarray(cases.F, dtype=np.float64).tobytes(),
                     bytes(cal), np.asarray(R, dtype=np.float64).tobytes(), np.asarray(t, dtype=np.float64).tobytes(),
                     np.array([radius], dtype=np.float64).tobytes(), np.array([use_orientation, 0], dtype=np.int32).tobytes()])
    imgs = b"".join(img.tobytes() for k in (cases.KF, cases.CF) for img in cases.images(k))
    (tmp_path / "in.bin").write_bytes(head + imgs)
    out = tmp_path / "out.bin"
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(out)])
    buf = out.read_bytes()
    counts = _lib.TemporalCounts.from_buffer_copy(buf, 0)
    off = ctypes.sizeof(_lib.TemporalCounts)
    ref = cases.case_reference(name, 1)
    fin = ref["final"]
    assert {k: getattr(counts, k) for k in ref["counts"]} == ref["counts"]
    n, n_kf = counts.n_final, counts.n_kf
    assert n > 1000 and cases.true_final(ref) > 1000
    for key, dtype, count in (("row_ptr", np.int32, n_kf + 1), ("cf_index", np.int32, n), ("left", orc.EDGE_DTYPE, n),
                              ("right", orc.EDGE_DTYPE, n), ("ncc_left", np.float64, n), ("sift_left", np.float64, n),
                              ("score_left", np.float64, n), ("score_right", np.float64, n), ("valid", np.uint8, n)):
        got = np.frombuffer(buf, dtype=dtype, count=count, offset=off)
        off += got.nbytes
        if key in ("left", "right"):
            assert oracle_chain._same_edges(got, fin[key]), key
        else:
            assert_bit_equal(got, fin[key], key)
    status = int(np.frombuffer(buf, dtype=np.int32, count=1, offset=off)[0])
    again = int(np.frombuffer(buf, dtype=np.int64, count=1, offset=off + 4)[0])
    assert off + 12 == len(buf)
    # the second match of the demo was not re-armed: today's search at the same radius
    assert status == 0 and again == cases.unprimed_reference(0, radius)["counts"]["n_candidates"] != counts.n_candidates
