#!/usr/bin/env python3
"""One regression per column (metrics.column_regress -> nm_column_regress) timed in one session, one process, three ways on
the same data:

  kernel   metrics.column_regress: one launch for all sets (pointer table, tables read where they lie)
  torch    the same estimator as batched fp64 tensor algebra on the same device, one set at a time (a set's centred design
           is [D, n, P] fp64): OLS by torch.linalg.solve on the normal equations of the centred design, Logit by the same
           Newton steps from zero with the same stopping rule, the largest step read back after every step
  numpy    the yardstick of the tests (tests/column_regress_ref.py) on the host, on copies made beforehand; with more than
           --numpy-max-sets sets only the first that many are fitted, and the record says so

for 1064 subjects, D = 32 (a latent space) and D = 379 (one modality), 1 / 20 / 256 sets, both kinds, q = 0 and 2 covariates.
Each leg: a warm-up call, then --repeats timed windows of some calls each, every window closed by a device synchronise; every
repeat is recorded, with min / median / max.  Before the timing the kernel's table of the first and the last set is held to the
yardstick's by the tests' closeness rule.  No ratio is a target: all three are recorded as they come.

One JSON document, to --out (default profiles/column_regress.json), with the clocks record of bench.py --full."""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np
import torch
import multi_modal_normative_modeling_amd as nm
from multi_modal_normative_modeling_amd import metrics
from bench import device_record, kernel_src_sha16
from tests import column_regress_ref as R

N = 1064


def stats(v):
    s = sorted(v)
    return {"min": s[0], "median": round((s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, 3), "max": s[-1]}


def make_sets(D, n_sets, q, kind, dev):
    rng = np.random.default_rng(1000 * D + 10 * n_sets + q + (5 if kind == "logit" else 0))
    pitch = (D + 3) // 4 * 4
    mats, ys, covs = [], [], []
    for _ in range(n_sets):
        x, y, cov = R.make_case(rng, N, D, q, kind)
        buf = torch.zeros(N, pitch, dtype=torch.float32)
        buf[:, :D] = torch.from_numpy(x)
        mats.append(buf.to(dev)[:, :D])
        ys.append(torch.from_numpy(y).to(dev))
        covs.append(torch.from_numpy(cov).to(dev) if q else None)
    return mats, ys, (covs if q else None)


def timed(fn, repeats, iters, dev):
    fn()
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize(dev)
        out.append(round((time.perf_counter() - t0) / iters * 1e3, 4))
    return out


def torch_set(x, y, cov, kind):
    """One set on the device in fp64: (coef, se_coef) per column by the kernel's estimator."""
    x, y = x.double(), y.double()
    n, D = x.shape
    cols = [torch.ones(D, n, 1, dtype=torch.float64, device=x.device), (x - x.mean(0)).t().unsqueeze(2)]
    if cov is not None:
        c = cov.double()
        cols.append((c - c.mean(0)).unsqueeze(0).expand(D, n, c.shape[1]))
    Z = torch.cat(cols, 2)                                         # [D, n, P]
    P = Z.shape[2]
    if kind == "ols":
        A = Z.transpose(1, 2) @ Z
        beta = torch.linalg.solve(A, Z.transpose(1, 2) @ y[None, :, None])
        rss = ((y[None, :, None] - Z @ beta) ** 2).sum((1, 2))
        C = torch.linalg.inv(A) * (rss / (n - P))[:, None, None]
        return beta[:, 1, 0], C[:, 1, 1].sqrt()
    beta = torch.zeros(D, P, 1, dtype=torch.float64, device=x.device)
    for _ in range(R.MAX_ITER):
        p = torch.sigmoid(Z @ beta)
        H = Z.transpose(1, 2) @ (Z * (p * (1 - p)))
        step = torch.linalg.solve(H, Z.transpose(1, 2) @ (y[None, :, None] - p))
        beta = beta + step
        if float(step.abs().max()) <= R.TOL:
            break
    p = torch.sigmoid(Z @ beta)
    C = torch.linalg.inv(Z.transpose(1, 2) @ (Z * (p * (1 - p))))
    return beta[:, 1, 0], C[:, 1, 1].sqrt()


def torch_leg(mats, ys, covs, kind):
    keep = None
    for k, m in enumerate(mats):
        keep = torch_set(m, ys[k], None if covs is None else covs[k], kind)
    return keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--widths", nargs="+", type=int, default=[32, 379])
    ap.add_argument("--sets", nargs="+", type=int, default=[1, 20, 256])
    ap.add_argument("--covariates", nargs="+", type=int, default=[0, 2])
    ap.add_argument("--kinds", nargs="+", type=str, default=["ols", "logit"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-max-sets", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "column_regress.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("at least three repeats per leg: the spread of the repeats is the record's only noise figure")
    dev = torch.device("cuda:0")
    out = {"tool": "bench_column_regress", "kernel_src_sha16": kernel_src_sha16(), "device": torch.cuda.get_device_name(dev),
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count, "subjects": N, "repeats": a.repeats,
           "unit": "milliseconds per call (all sets)", "shapes": {}}
    for kind in a.kinds:
        for q in a.covariates:
            for D in a.widths:
                for n_sets in a.sets:
                    mats, ys, covs = make_sets(D, n_sets, q, kind, dev)
                    call = lambda: metrics.column_regress(mats, ys, kind=kind, covariates=covs, device=dev)
                    got = call().cpu().numpy()
                    host = [(m.cpu().numpy(), y.cpu().numpy(), None if covs is None else covs[k].cpu().numpy())
                            for k, (m, y) in enumerate(zip(mats, ys))]
                    for k in sorted({0, n_sets - 1}):              # the timed kernel computes what the yardstick computes
                        worst = R.close(got[k], R.table(*host[k], None, kind))
                        if not worst <= 1.0:
                            raise SystemExit(f"{kind} q={q} D={D}, {n_sets} sets: set {k} differs from the yardstick ({worst})")
                    entry = {"fits": D * n_sets, "n_iter_max": int(got[:, :, 7].max())}
                    iters = max(1, min(50, 1000 // n_sets))
                    v = timed(call, a.repeats, iters, dev)
                    entry["kernel"] = {"ms": v, "calls_per_window": iters, **stats(v)}
                    iters_t = max(1, min(10, 20 // n_sets))
                    v = timed(lambda: torch_leg(mats, ys, covs, kind), a.repeats, iters_t, dev)
                    entry["torch_fp64_batched"] = {"ms": v, "calls_per_window": iters_t, **stats(v)}
                    part = host[:a.numpy_max_sets]
                    v = []
                    for _ in range(a.repeats if len(part) * D <= 1000 else 3):
                        t0 = time.perf_counter()
                        for x, y, c in part:
                            R.table(x, y, c, None, kind)
                        v.append(round((time.perf_counter() - t0) * 1e3, 2))
                    entry["numpy_host"] = {"ms": v, "sets_fitted": len(part), **stats(v)}
                    out["shapes"][f"{kind}_q{q}_D{D}_{n_sets}"] = entry
                    print(f"{kind} q={q} D={D} x {n_sets} sets: kernel {entry['kernel']['median']} ms, torch "
                          f"{entry['torch_fp64_batched']['median']} ms, numpy {entry['numpy_host']['median']} ms for {len(part)} sets",
                          flush=True)
                    del mats, ys, covs, host, part
                    torch.cuda.empty_cache()
    # the clocks this run saw (bench.py --full's record), from a short traced train launch of a small set
    from bench_latent import make_set, SHAPES
    out["clocks"] = device_record(torch, nm, make_set(SHAPES["SE-3"], 1, dev), dev)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
