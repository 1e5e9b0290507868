#!/usr/bin/env python3
"""GPU diagnostic (not part of the suite): the random-shape comparison of tests/test_gpu_fuzz.py over many more seeds, or --
with --twin NAME -- the twin comparison of tests/test_gpu_twins.py on draw(NAME, seed) for --first / --count seeds.
The twin run collects assertion failures and prints the failing cases; the first error that is not an assertion failure (a
launch status, a HIP error: the device may have faulted) ends the run at once, nothing more is started on the GPU."""
import argparse, sys, traceback
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ap = argparse.ArgumentParser()
ap.add_argument("--first", type=int, default=1000)
ap.add_argument("--count", type=int, default=150)
ap.add_argument("--twin", choices=("plain", "devpass", "devpass_multi", "latent", "split"), default=None)
a = ap.parse_args()
bad = []
if a.twin is not None:
    from tests.twin_cases import draw
    from tests.test_gpu_twins import run
    for seed in range(a.first, a.first + a.count):
        cs = draw(a.twin, seed)
        try:
            run(cs)
        except AssertionError as e:             # a twin that disagrees: collect, go on
            bad.append((seed, cs, str(e)[:300]))
        except BaseException:                   # noqa: BLE001 -- anything else: stop here, start nothing more on the GPU
            traceback.print_exc()
            print(f"STOPPED at seed {seed}: {cs}")
            for b in bad:
                print("FAILED", b)
            sys.exit(2)
    print(f"{a.count - len(bad)} / {a.count} {a.twin} cases ok")
    for b in bad:
        print("FAILED", b)
    sys.exit(1 if bad else 0)

from tests.test_gpu_fuzz import _draw
from tests.test_gpu_fullsize import run_case
for seed in range(a.first, a.first + a.count):
    dims, Z, combine, B, hidden, c_dim, non_linear = _draw(seed)
    try:
        run_case(dims, Z, combine, B, seed=seed, hidden=tuple(hidden), c_dim=c_dim, non_linear=non_linear,
                 ll32_tol=1e-4 * max(1.0, (256.0 / B) ** 0.5))
    except Exception as e:                      # noqa: BLE001 -- diagnostic: collect and report every failing shape
        bad.append((seed, dims, Z, combine, B, hidden, c_dim, non_linear, repr(e)[:200]))
print(f"{a.count - len(bad)} / {a.count} shapes ok")
for b in bad:
    print("FAILED", b)
sys.exit(1 if bad else 0)
