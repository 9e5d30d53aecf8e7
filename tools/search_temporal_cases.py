"""CPU search for the boxed frames of tests/temporal_cases.py: which kept box of the 120x200 scene leaves a mate count on
the work units of the temporal kernels (16 mates per block and 4 per wave in temporal_candidates, 16 quads per block in
ncc_quads_indexed), and the smallest non-empty counts.  Prints candidates; the chosen ones are committed as constants in
tests/temporal_cases.py and re-derived by tests/test_temporal_cases.py.

    python tools/search_temporal_cases.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import temporal_cases as tc  # noqa: E402


def count(k, box):
    name = f"search-{k}-{box}"
    tc.add_boxed({name: (*tc.SMALL, k, box)})
    return len(tc.oracle_mates(name)[0])


def main():
    h, w = tc.SMALL
    for k in (0, 2):
        seen = {}
        for x1 in range(24, w + 1, 2):
            n = count(k, (0, h, 0, x1))
            seen.setdefault(n % 16, (n, x1))
        print(f"frame {k}: n % 16 -> (n, x1) of box (0, {h}, 0, x1):", {m: seen[m] for m in sorted(seen)})
        small = {}
        for size in (16, 20, 24, 28, 32):
            for y0 in range(8, h - size, 12):
                for x0 in range(8, w - size, 12):
                    n = count(k, (y0, y0 + size, x0, x0 + size))
                    if 0 < n < 16:
                        small.setdefault(n, (y0, y0 + size, x0, x0 + size))
        print(f"frame {k}: smallest non-empty counts -> box:", {n: small[n] for n in sorted(small)})


if __name__ == "__main__":
    main()
