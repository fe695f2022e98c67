"""CPU: the search that chose the seeds of tests/second_order_cases.py (SEEDS) for the large shapes.

    python tools/second_order_case_seeds.py m208 400000 200 [first_seed]

A case has two draws, ``sw_shaped_system(seed + i)``, and has to pass tests/test_second_order_reference.py -- above all its conditioning
check, which asks for an amplification below 10 and which the median draw of the generator misses by a factor of 4 to 6 from n = 28 on.
The check costs a second or more per seed, so the seeds are ranked first by a proxy that costs a millisecond: the larger, over the two
draws, of cond(M) max(1, cond(M + C) / 10) with M = B + C T* -- the two matrices the coefficient blocks are solved with.  The best
``top`` consecutive pairs among ``count`` seeds are then put through the checks of the reference test; the first that passes is
printed.  What this finds are ATYPICALLY WELL-CONDITIONED draws, by construction."""
import contextlib
import io
import os
import sys
from concurrent.futures import ProcessPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from geconpy_amd import workloads as wl
from tests import second_order_cases as sc
from tests import test_second_order_reference as tr


def proxies(args):
    base, lo, hi = args
    n, s, nl, k, _, _ = sc.SHAPES[base][0]
    out = []
    for seed in range(lo, hi):
        _, B, C, _, T_star = wl.sw_shaped_system(seed, n, s, nl, k)
        M = B + C @ T_star
        out.append(np.linalg.cond(M) * max(1.0, np.linalg.cond(M + C) / 10.0))
    return out


def passes(args):
    """The conditions of the reference test on the case, its variants and its nested models, with this seed."""
    base, seed = args
    sc.SEEDS[base] = seed
    sc.problem.cache_clear()
    sc.reference.cache_clear()
    names = [name for name in tr.PROBLEMS if name == base or (name not in sc.SHAPES and name.startswith(base + "_"))]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            for name in names:
                tr.test_conditioning_of_every_draw(name)
                tr.test_second_order_terms_are_visible_and_logp_does_not_cancel(name)
    except AssertionError:
        return seed, False
    return seed, True


def main(base, count, top, first=30000, workers=min(8, os.cpu_count() or 1)):
    with ProcessPoolExecutor(workers) as ex:
        c = np.concatenate(list(ex.map(proxies, [(base, a, min(a + 500, first + count)) for a in range(first, first + count, 500)])))
        pair = np.maximum(c[:-1], c[1:])
        order = np.argsort(pair)[:top]
        print(f"{base}: proxy median {np.median(c):.0f}, best pairs {np.round(pair[order[:5]], 1)}")
        for seed, ok in ex.map(passes, [(base, first + int(j)) for j in order]):
            if ok:
                print("seed", seed)
                return seed
    print("no seed among the best", top)
    return None


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), *(int(x) for x in sys.argv[4:5]))
