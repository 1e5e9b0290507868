"""Numpy restatement of the posterior-predictive fold (nm_devpass_draws, include/nmhip.h): the running mean / M2 over the S
reconstructions of an element in draw order, in fp32 with every operation rounded on its own, and the exports derived from
them.  Pure numpy: no device, no library call (sense_inputs alone builds torch tensors, the sense test's tables and weights).
The GPU tests hold the kernel to this, bit for bit where the definition is only subtraction, multiplication and addition."""
import numpy as np

F = np.float32
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# The sense test's model (tests/test_gpu_devpass_draws.py on the device, tests/test_predictive_ref_cpu.py on the oracle): shape A
# of the deviation-pass tests with linear layers -- the decoders are then affine in z, so the mean over independent draws
# tends to the noise-free reconstruction at the 1 / sqrt(S) rate with no curvature term on top.
SENSE = {"N": 300, "dims": (61, 90, 47), "hidden": (64, 48), "Z": 12, "c_dim": 3, "combine": "gpoe", "non_linear": False,
         "init_seed": 31, "data_seed": 21}


def sense_inputs():
    """(xs, cs, state) of the sense test: the tables and the weights, the same on the device and on the oracle."""
    import torch
    from multi_modal_normative_modeling_amd.layout import ModelSpec, ParamLayout
    c = SENSE
    g = torch.Generator().manual_seed(c["data_seed"])
    xs = [torch.randn(c["N"], d, generator=g) * 1.1 for d in c["dims"]]
    cov = torch.zeros(c["N"], c["c_dim"])
    cov[torch.arange(c["N"]), torch.randint(0, c["c_dim"], (c["N"],), generator=g)] = 1
    spec = ModelSpec(list(c["dims"]), list(c["hidden"]), c["Z"], c["c_dim"], c["non_linear"], "multimodal")
    return xs, [cov] * len(c["dims"]), ParamLayout(spec).init_reference_rule(c["init_seed"])


def draw_seeds(seed, n_draws):
    """Draw 0: the job's seed; draw s: (seed + s * 0x9E3779B97F4A7C15) mod 2^64."""
    return [(int(seed) + s * GOLDEN) & MASK64 for s in range(int(n_draws))]


def fold(xhats):
    """xhats: [S, ...] fp32 reconstructions in draw order -> (mean, M2), fp32."""
    xh = np.asarray(xhats, dtype=F)
    mean = xh[0].copy()
    m2 = np.zeros_like(mean)
    for s in range(1, xh.shape[0]):
        rs = F(1.0) / F(s + 1)
        d = xh[s] - mean
        mean = mean + d * rs
        m2 = m2 + d * (xh[s] - mean)
    return mean.astype(F), m2.astype(F)


def variance(m2, S):
    """pred_var = M2 * v, v = 1 / (S - 1) in fp32 (S = 1: 0)."""
    v = F(1.0) / F(S - 1) if S > 1 else F(0.0)
    return (np.asarray(m2, dtype=F) * v).astype(F)


def msq(x, mean, var, S):
    """pred_msq = e * e + pred_var * c, e = x - mean, c = (S - 1) / S in fp32."""
    c = F(S - 1) / F(S)
    e = np.asarray(x, dtype=F) - np.asarray(mean, dtype=F)
    return (e * e + np.asarray(var, dtype=F) * c).astype(F)


def zscore(x, mean, var, noise_var):
    """pred_z = e / sqrt(noise_var + pred_var)."""
    e = np.asarray(x, dtype=F) - np.asarray(mean, dtype=F)
    return (e / np.sqrt(np.asarray(noise_var, dtype=F) + np.asarray(var, dtype=F))).astype(F)


def exports(xhats, x, noise_var):
    """Everything the pass exports for one decoder from the S reconstructions [S, N, D], the inputs [N, D] and the
    observation variance [D]: a dict of fp32 arrays (the row means in fp64 accumulation: the kernel's own summation order
    is held to them within the sibling's tolerance, not bit for bit)."""
    S = len(xhats)
    mean, m2 = fold(xhats)
    var = variance(m2, S)
    q = msq(x, mean, var, S)
    z = zscore(x, mean, var, noise_var)
    return {"mean": mean, "var": var, "msq": q, "z": z,
            "rowdev": q.astype(np.float64).mean(axis=1).astype(F), "rowz2": (z.astype(np.float64) ** 2).mean(axis=1).astype(F)}
