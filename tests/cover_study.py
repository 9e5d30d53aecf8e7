"""The study of the keyframe coverage along a trajectory (asserted in tests/test_cover_oracle.py): the twelve
noisy scenes of tests/depth_scenes.py extended to eight frames, the oracle's record per frame at the planted pose and at the
planted pose turned by the perturbation of the alignment's study (tests/align_scenes.py::perturbed: 0.34 degrees, 27 mm)."""
import functools

from tests import align_scenes as asc
from tests import depth_scenes as ds
from tests import oracle_cover as ocv

FRAMES = 8


def shares(r):
    """(in-frame share of the live mates, associated share of those in frame, explained share of the current edges, covered
    share of the cells that hold edges, median displacement bin, decision under the default policy)"""
    live = r["n_kf"] - r["n_dead"]
    return (r["n_in_frame"] / live if live else 0.0, r["n_assoc"] / r["n_in_frame"] if r["n_in_frame"] else 0.0,
            r["n_explained"] / r["n_edges"] if r["n_edges"] else 0.0, r["n_cells_covered"] / r["n_cells_cur"] if r["n_cells_cur"] else 0.0,
            r["disp_median_bin"], ocv.decide(r)[0])


@functools.lru_cache(maxsize=None)
def rows(k):
    """[(shares at the planted pose, shares at the perturbed pose)] for frames 1 .. FRAMES of noisy scene k"""
    rig, seed, kind, sigma, clutter = ds.NOISY[k]
    sc = ds.scene(rig, seed, kind, sigma, clutter, sigma_disp=ds.SIGMA_DISP, frames=FRAMES)
    out = []
    for (R, t), (E0, _) in zip(sc["poses"], sc["frames"]):
        at = [ocv.cover(sc["kf_left"], sc["kf_right"], None, E0, ds.W, ds.H, sc["calib"], Rp, tp) for Rp, tp in ((R, t), asc.perturbed(R, t))]
        out.append(tuple(shares(r) for r in at))
    return out


if __name__ == "__main__":
    for k, row in enumerate(ds.NOISY):
        print(k, row)
        for f, (a, b) in enumerate(rows(k), 1):
            print(f"  frame {f}: planted  in {a[0]:.3f} assoc {a[1]:.3f} expl {a[2]:.3f} cells {a[3]:.3f} bin {a[4]:2d} dec {a[5]} | "
                  f"perturbed in {b[0]:.3f} assoc {b[1]:.3f} expl {b[2]:.3f} cells {b[3]:.3f} bin {b[4]:2d} dec {b[5]}")
