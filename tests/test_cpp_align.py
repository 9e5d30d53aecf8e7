"""The edge alignment through the C++ adapter (include/ebvo/adapters.hpp: MotionTrackerHIP::align_Relative_Pose):
tests/cpp/align_demo.cpp compiles against the C ABI alone and prints the defaults of the Python binding; on a GPU it returns the
oracle's pose bits, result fields and associations on a tiny case of tests/align_cases.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from edge_based_visual_odometry_amd.api import Context
from tests import align_cases as ac
from tests import oracle_align as oa
from tests.util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_demo(tmp_path):
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "align_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "align_demo.cpp"), "-o", exe, "-L", libdir, "-lebvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_demo_builds_with_plain_gxx_and_prints_the_defaults(tmp_path):
    words = subprocess.check_output([build_demo(tmp_path)], text=True).split()
    got = {k: float(v) for k, v in zip(words[0::2], words[1::2])}
    p = _lib.AlignParams()
    _lib.load_library().ebvo_align_default_params(ctypes.byref(p))
    assert got == {name: float(getattr(p, name)) for name, _ in p._fields_}
    assert {k: got[k] for k in oa.DEFAULTS} == {k: float(v) for k, v in oa.DEFAULTS.items()} and got["block_threads"] == 0


@pytest.mark.gpu
def test_adapter_returns_the_bits_of_the_oracle(tmp_path):
    """the mates and edge lists of a tiny case read from files: the pose bits, the result fields and both association arrays
    equal the oracle's"""
    exe = build_demo(tmp_path)
    case = ac.cases()["n_kf_65"]()
    ref = ac.run_oracle(case)
    names = []
    for k in ("kf_left", "kf_right", "edges_left", "edges_right"):
        p = tmp_path / f"{k}.bin"
        p.write_bytes(np.ascontiguousarray(case[k], dtype=_lib.EDGE_DTYPE).tobytes())
        names.append(str(p))
    cal = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in case["calib"]] +
                         [np.asarray(case["R0"], dtype=np.float64).reshape(-1), np.asarray(case["t0"], dtype=np.float64).reshape(-1)])
    (tmp_path / "pose.bin").write_bytes(cal.tobytes())
    out = tmp_path / "out.bin"
    p = case["params"]
    subprocess.check_call([exe, *names, str(tmp_path / "pose.bin"), str(case["img_w"]), str(case["img_h"]), str(p["rounds"]),
                           str(p["iterations"]), str(out)])
    buf = out.read_bytes()
    res = _lib.AlignedPose.from_buffer_copy(buf, 0)
    n = len(case["kf_left"])
    off = ctypes.sizeof(_lib.AlignedPose)
    aL = np.frombuffer(buf, dtype=np.int32, count=n, offset=off)
    aR = np.frombuffer(buf, dtype=np.int32, count=n, offset=off + 4 * n)
    assert off + 8 * n == len(buf)
    got = Context._aligned_dict(res, aL, aR)
    for k in ("status", "stop_reason", "rounds_run", "steps_kept", "n_kf", "fit_terms", "inliers", "n_assoc"):
        assert got[k] == ref[k], k
    for k in ("cost_first", "cost_last", "rms_normal", "R", "t", "assoc_left", "assoc_right"):
        assert_bit_equal(np.asarray(got[k]), np.asarray(ref[k]), k)
    assert got["status"] == 0 and got["steps_kept"] > 0 and got["n_assoc"] == (65, 65)
