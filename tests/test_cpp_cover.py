"""The keyframe coverage and the switch policy through the C++ adapter (include/ebvo/adapters.hpp:
MotionTrackerHIP::keyframe_Coverage / should_Switch_Keyframe): tests/cpp/cover_demo.cpp compiles against the C ABI alone and
prints the defaults of both parameter structs of the Python binding; on a GPU it returns the oracle's bits on a small scene case
of tests/cover_cases.py, on Gamma / lambda and on the triangulated Gamma."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from tests import cover_cases as cc
from tests import oracle_cover as ocv
from tests.util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_demo(tmp_path):
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "cover_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cover_demo.cpp"), "-o", exe, "-L", libdir, "-lebvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_demo_builds_with_plain_gxx_and_prints_the_defaults(tmp_path):
    lines = subprocess.check_output([build_demo(tmp_path)], text=True).strip().split("\n")
    assert len(lines) == 2
    got = [{k: float(v) for k, v in zip(w[0::2], w[1::2])} for w in (line.split() for line in lines)]
    lib = _lib.load_library()
    p, q = _lib.CoverParams(), _lib.KeyframePolicy()
    lib.ebvo_cover_default_params(ctypes.byref(p))
    lib.ebvo_keyframe_policy_default(ctypes.byref(q))
    assert got[0] == {name: float(getattr(p, name)) for name, _ in p._fields_}
    assert got[1] == {name: float(getattr(q, name)) for name, _ in q._fields_}
    assert {k: got[0][k] for k in ocv.DEFAULTS} == {k: float(v) for k, v in ocv.DEFAULTS.items()} and got[0]["reserved"] == 0
    assert got[1] == {k: float(v) for k, v in ocv.POLICY.items()}


@pytest.mark.gpu
def test_adapter_returns_the_bits_of_the_oracle(tmp_path):
    exe = build_demo(tmp_path)
    case = cc.curves("euroc", lambda_=True, n_kf=300)
    refs = (cc.run_oracle(case, cover_cell=24), cc.run_oracle(dict(case, lambda_=None), cover_cell=24))
    names = {}
    for k in ("kf_left", "kf_right", "edges_left"):
        p = tmp_path / f"{k}.bin"
        p.write_bytes(np.ascontiguousarray(case[k], dtype=_lib.EDGE_DTYPE).tobytes())
        names[k] = str(p)
    (tmp_path / "lambda.bin").write_bytes(np.asarray(case["lambda_"], dtype=np.float64).tobytes())
    cal = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in case["calib"]] +
                         [np.asarray(case["R"], dtype=np.float64).reshape(-1), np.asarray(case["t"], dtype=np.float64).reshape(-1)])
    (tmp_path / "pose.bin").write_bytes(cal.tobytes())
    out = tmp_path / "out.bin"
    subprocess.check_call([exe, names["kf_left"], names["kf_right"], str(tmp_path / "lambda.bin"), names["edges_left"],
                           str(tmp_path / "pose.bin"), str(case["img_w"]), str(case["img_h"]), "24", str(out)])
    buf = out.read_bytes()
    n, n0, rs = len(case["kf_left"]), len(case["edges_left"]), ctypes.sizeof(_lib.KeyframeCover)
    nc = refs[0]["cw"] * refs[0]["ch"]
    per = rs + 8 + 8 * n + 4 * n + 8 * nc + n + n0
    assert len(buf) == 2 * per
    for k, ref in enumerate(refs):
        o = k * per
        r = _lib.KeyframeCover.from_buffer_copy(buf, o)
        for f in ocv.INT_FIELDS:
            assert getattr(r, f) == ref[f], (k, f)
        assert_bit_equal(np.array(r.hist[:], dtype=np.int32), ref["hist"], f"pass {k} hist")
        o += rs
        assert tuple(np.frombuffer(buf, dtype=np.int32, count=2, offset=o)) == ocv.decide(ref), f"pass {k} decision"
        o += 8
        assert_bit_equal(np.frombuffer(buf, dtype=np.float64, count=n, offset=o), ref["disp"], f"pass {k} disp")
        o += 8 * n
        assert_bit_equal(np.frombuffer(buf, dtype=np.int32, count=n, offset=o), ref["assoc"], f"pass {k} assoc")
        o += 4 * n
        assert_bit_equal(np.frombuffer(buf, dtype=np.int32, count=nc, offset=o), ref["cell_edges"], f"pass {k} cell_edges")
        o += 4 * nc
        assert_bit_equal(np.frombuffer(buf, dtype=np.int32, count=nc, offset=o), ref["cell_explained"], f"pass {k} cell_explained")
        o += 4 * nc
        assert_bit_equal(np.frombuffer(buf, dtype=np.uint8, count=n, offset=o), ref["flags"], f"pass {k} flags")
        o += n
        assert_bit_equal(np.frombuffer(buf, dtype=np.uint8, count=n0, offset=o), ref["explained"], f"pass {k} explained")
    assert refs[0]["n_assoc"] > 100 and refs[0]["disp"].tobytes() != refs[1]["disp"].tobytes()
