"""The handover of the depths on promotion through the C++ adapter (include/ebvo/adapters.hpp:
MotionTrackerHIP::carry_Mate_Depths): tests/cpp/carry_demo.cpp compiles against the C ABI alone and prints the defaults of the
Python binding; on a GPU it returns the oracle's bits on a small case of tests/carry_cases.py, with the old state and without."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from tests import carry_cases as cc
from tests import oracle_carry as oc
from tests.util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_demo(tmp_path):
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "carry_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "carry_demo.cpp"), "-o", exe, "-L", libdir, "-lebvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_demo_builds_with_plain_gxx_and_prints_the_defaults(tmp_path):
    words = subprocess.check_output([build_demo(tmp_path)], text=True).split()
    got = {k: float(v) for k, v in zip(words[0::2], words[1::2])}
    p = _lib.DepthCarryParams()
    _lib.load_library().ebvo_depth_carry_default_params(ctypes.byref(p))
    assert got == {name: float(getattr(p, name)) for name, _ in p._fields_}
    assert {k: got[k] for k in oc.DEFAULTS} == {k: float(v) for k, v in oc.DEFAULTS.items()} and got["reserved"] == 0


@pytest.mark.gpu
def test_adapter_returns_the_bits_of_the_oracle(tmp_path):
    exe = build_demo(tmp_path)
    case = cc.curves("euroc", 300, 300)
    refs = (cc.run_oracle(case, carry=0.75), cc.run_oracle(dict(case, state=None), carry=0.75))
    names = {}
    for k in ("kf_left", "kf_right", "new_left", "new_right"):
        p = tmp_path / f"{k}.bin"
        p.write_bytes(np.ascontiguousarray(case[k], dtype=_lib.EDGE_DTYPE).tobytes())
        names[k] = str(p)
    lam, info, nobs = case["state"]
    (tmp_path / "state.bin").write_bytes(np.asarray(lam, dtype=np.float64).tobytes() + np.asarray(info, dtype=np.float64).tobytes() +
                                         np.asarray(nobs, dtype=np.int32).tobytes())
    cal = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in case["calib"]] +
                         [np.asarray(case["R"], dtype=np.float64).reshape(-1), np.asarray(case["t"], dtype=np.float64).reshape(-1)])
    (tmp_path / "pose.bin").write_bytes(cal.tobytes())
    out = tmp_path / "out.bin"
    subprocess.check_call([exe, names["kf_left"], names["kf_right"], str(tmp_path / "state.bin"), names["new_left"], names["new_right"],
                           str(tmp_path / "pose.bin"), str(case["img_w"]), str(case["img_h"]), "0.75", str(out)])
    buf = out.read_bytes()
    n, rs = len(case["new_left"]), ctypes.sizeof(_lib.DepthCarried)
    per = rs + 8 * n + 8 * n + 4 * n + 4 * n + n
    assert len(buf) == 2 * per
    for k, ref in enumerate(refs):
        o = k * per
        r = _lib.DepthCarried.from_buffer_copy(buf, o)
        for f in oc.INT_FIELDS:
            assert getattr(r, f) == ref[f], (k, f)
        assert_bit_equal(np.frombuffer(buf, dtype=np.float64, count=n, offset=o + rs), ref["lambda_"], f"pass {k} lambda")
        assert_bit_equal(np.frombuffer(buf, dtype=np.float64, count=n, offset=o + rs + 8 * n), ref["info"], f"pass {k} info")
        assert_bit_equal(np.frombuffer(buf, dtype=np.int32, count=n, offset=o + rs + 16 * n), ref["n_obs"], f"pass {k} n_obs")
        assert_bit_equal(np.frombuffer(buf, dtype=np.int32, count=n, offset=o + rs + 20 * n), ref["src_index"], f"pass {k} src_index")
        assert_bit_equal(np.frombuffer(buf, dtype=np.uint8, count=n, offset=o + rs + 24 * n), ref["flags"], f"pass {k} flags")
    assert refs[0]["n_carried"] > 100 and refs[1]["n_assoc"] == 0
