"""CPU search for the pairs of tests/finalize_cases.py: which widths of the s2 pair give kept rows of exactly 64 and of more
(into the Best-Nearly-Best test, and with bnb_ratio = 0 into the clustering), which low 752-wide crop gives rows of more
than 256 with two equal scores while the oracle chain stays under ten seconds, and which small crops have an edge count
of 0, 1 and 255 modulo 256.  Prints candidates; the chosen ones are committed as constants in tests/finalize_cases.py and
re-derived by tests/test_finalize_cases.py.

    python tools/search_finalize_cases.py [long64] [long256] [nl]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tests import finalize_cases as fc  # noqa: E402
from tests import oracle as orc  # noqa: E402
from tests import oracle_chain  # noqa: E402


def bnb_rows(name, ratio):
    """row lengths after the Best-Nearly-Best test on the NCC scores (what enters the clustering without SIFT)"""
    s = fc.stage1(name)
    k = s["keep"].astype(bool)
    rp = oracle_chain.filter_rows(s["row_ptr"], k)
    cnt, _ = orc.bnb_test(rp, s["best"][k], ratio, True)
    return np.asarray(cnt)


def long64():
    for scene in (7, 11):
        for w in range(150, 200):
            name = f"search-long64-{scene}-{w}"
            fc.add_pairs({name: (96, w, dict(scene=scene), fc.ALL_KEPT)})
            rows = fc.kept_rows(name)
            if not ((rows == 64).any() and (rows > 64).any()):
                continue
            b = bnb_rows(name, 0.0)
            print(f"scene {scene} 96x{w}: kept rows ==64: {(rows == 64).sum()}, >64: {(rows > 64).sum()}, longest {rows.max()}; "
                  f"after bnb_ratio 0 ==64: {(b == 64).sum()}, >64: {(b > 64).sum()}", flush=True)


def long256():
    for h in range(24, 33):
        name = f"search-long256-{h}"
        fc.add_pairs({name: (h, 752, {}, fc.ALL_KEPT)})
        c = fc.conditions(name)
        ties = fc.rows_with_equal_scores(name, 256) if c["rows_over_256"] else []
        t0 = time.time()
        counts = fc.chain(name)["counts"] if c["n_pairs"] < 600000 else None
        print(f"{h}x752: {c}, rows over 256 with equal scores: {len(ties)}, chain {time.time() - t0:.1f} s: {counts}", flush=True)


def nl():
    seen = {}
    for h in range(36, 60, 2):
        for w in range(64, 161):
            name = f"search-nl-{h}-{w}"
            fc.add_pairs({name: (h, w, {}, {})})
            n = len(fc.toed_left(name))
            if n % 256 in (0, 1, 255) and n > 0:
                seen.setdefault(n % 256, []).append((h, w, n))
    print("n_left % 256 -> (h, w, n_left):", seen, flush=True)


if __name__ == "__main__":
    todo = sys.argv[1:] or ["long64", "long256", "nl"]
    for what in todo:
        {"long64": long64, "long256": long256, "nl": nl}[what]()
