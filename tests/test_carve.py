"""csrc/ebvo_carve.h, the layout of the host-array calls' staging buffer, checked by a stand-alone host program
(tests/cpp/carve_check.cpp): element counts 0, 1, 3, 63, 64, 65 and 2^31 - 1 of 1, 4, 8 and sizeof(ebvo_edge) bytes."""
import os
import subprocess

from edge_based_visual_odometry_amd._lib import EDGE_DTYPE


def test_carve_layout(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "carve_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I",
                           os.path.join(root, "edge_based_visual_odometry_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "carve_check.cpp"), "-o", exe])
    out = subprocess.run([exe, str(EDGE_DTYPE.itemsize)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout
