"""Post-hoc metrics on the device: host side of csrc/nm_metrics.hip.

`posthoc_metrics` = compute_classification_performance(method='roc') of
multimodal_kfold_cvae_group_analysis_1x1.py:105-157 for many score sets at once (one workgroup per set);
`confusion_metrics` = evaluate() of multimodal_kfold_cvae_nmpmcont.py:29-70 from hard predictions.
Scores stay on the GPU (they are the per-subject mean deviations the forward pass exported); only the
[n_sets, 8] fp64 result table comes back.
`roi_effect` = cliff_delta of utils.py:97-109 for every ROI column of many tables at once (one workgroup per table and
64 columns), on the ROI-wise squared errors where the evaluation jobs exported them; `cliff_delta` is the reference's
signature on top of it.  `roi_significance` = the Mann-Whitney test per ROI column of the same tables with its
Benjamini-Hochberg q and the max-statistic label-permutation test; `mann_whitney` is scipy's two-sample signature on top of it.
`auc_bootstrap` = the per-subject ROC-AUC of many score sets with its stratified-bootstrap percentile interval, and the paired
comparison of sets that share subjects; `auc_compare` is the two-procedure convenience on top of it.
`column_regress` = one OLS or Logit fit per column of many tables at once (target ~ const + column + covariates, the Wald
p-values of both reported parameters); `latent_pvalues` is the reference's signature (utils_vae.py:163-174) on top of it.
`operating_points` = every threshold rule of compute_classification_performance (roc, f1, pr, cost, eer; f1max and spec besides)
selected on one score set and scored on another, with PR-AUC, partial AUC and the ROC on a grid per set;
`classification_performance` is the reference's signature (group_analysis_1x1.py:105-157) on top of it.
`cohort_moments` / `normative_z` = the normative z-map: per ROI column the reference cohort's mean and sd, every subject's
z-score against them with the per-subject extreme-deviation counts and the per-ROI extreme-deviation map; `cohort_cov` /
`mahalanobis` = the full-covariance counterpart in latent space (the sigma-normalised extra of SURVEY.md, never the parity output).
`fit_quality` = the model's fit per ROI on the hold-out controls, with no patient label: Pearson and Spearman rho, SMSE, EXPV,
MSLL against the trivial train-moments model, RMSE, and the shape of the z distribution (bias, sd, skewness, kurtosis, coverage).
`cohort_quantiles` / `normative_centile` = the normative centiles: per ROI column the reference cohort's quantiles, median and MAD,
and every subject's percentile rank in that cohort (with an exact leave-one-out form), the per-subject counts in the tails and the
per-ROI extreme-centile map; `robust_moments` turns median and MAD into a moments table for `normative_z`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .engine import _stream_ptr, require_gpu

POSTHOC_COLUMNS = ("roc_auc", "threshold", "accuracy", "recall", "specificity", "significance_ratio", "n_pos", "n_neg")
CONFUSION_COLUMNS = ("accuracy", "auroc", "sensitivity", "specificity", "f1_score", "precision", "n_pos", "n_neg")
ROI_EFFECT_COLUMNS = ("cliff_delta", "auc", "n_more", "n_less", "n_x", "n_y", "mean_x", "mean_y")
ROI_SIGNIFICANCE_COLUMNS = ("u_x", "tie_term", "z", "p_mwu", "q_bh", "p_perm", "p_maxt", "n_perm")
COLUMN_REGRESS_COLUMNS = ("const", "coef", "se_const", "se_coef", "p_const", "p_coef", "n_obs", "n_iter")
# the row export of the likelihood pass (nm_devpass_iw, JobSet.forward_loglik): NM_IW_ROW_COLUMNS values per subject
LOGLIK_ROW_COLUMNS = ("log_px", "elbo", "ess", "kl_mc", "kl", "recon_ll", "logw_max", "logw_min")
assert len(LOGLIK_ROW_COLUMNS) == _lib.NM_IW_ROW_COLUMNS
# the row export of the end-to-end model's evaluation pass (nm_e2e_pass, JobSet.forward_endtoend): NM_E2E_ROW_COLUMNS values
# per subject -- class probability, hard prediction, logit margin, mean deviation under the health / disease decoder bank and
# their difference (positive: the disease bank fits the subject better), the analytic KL, status 0 / 1 (a non-finite value)
ENDTOEND_ROW_COLUMNS = ("p_disease", "pred", "margin", "dev_health", "dev_disease", "contrast", "kl", "status")
assert len(ENDTOEND_ROW_COLUMNS) == _lib.NM_E2E_ROW_COLUMNS
# the row export of the regression model's evaluation pass (nm_fi_pass, JobSet.forward_fi): NM_FI_ROW_COLUMNS values per
# subject -- mean, standard deviation, minimum and maximum of the S FI predictions (one per latent draw), the mean's error
# against the target, the mean deviation over the decoders (draw 0), the analytic KL, status (1: a non-finite value,
# 2: no target, 3: both).  fi_sd is the spread the latent draw alone causes, not a predictive interval
FI_ROW_COLUMNS = ("fi_pred", "fi_sd", "fi_min", "fi_max", "err", "dev", "kl", "status")
assert len(FI_ROW_COLUMNS) == _lib.NM_FI_ROW_COLUMNS
# a row of the normative chart (engine.JobSet.chart, nm_chart_pass): per (cell, ROI) the mean and the unbiased variance of
# x_hat over the request's latent rows, the row count, and status 0 / -2 (fewer than two rows, or a non-finite value)
CHART_COLUMNS = ("mean", "var_latent", "n_rows", "status")
assert len(CHART_COLUMNS) == _lib.NM_CHART_COLUMNS
COLUMN_REGRESS_KINDS = {"ols": _lib.NM_REG_OLS, "logit": _lib.NM_REG_LOGIT}


def _segments(parts: Sequence[torch.Tensor], device, dtype):
    sizes = [int(p.numel()) for p in parts]
    if not sizes:
        raise ValueError("no score sets")
    off = torch.zeros(len(sizes) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0).to(torch.int32)
    flat = torch.cat([p.reshape(-1).to(device=device, dtype=dtype) for p in parts]) if sum(sizes) else \
        torch.zeros(1, dtype=dtype, device=device)
    return flat.contiguous(), off.to(device), sizes


def posthoc_metrics(scores: Sequence[torch.Tensor], positive: Sequence[torch.Tensor],
                    thresholds: Optional[Sequence[float]] = None, device="cuda:0") -> torch.Tensor:
    """One row per set: roc_auc, threshold (Youden's J unless given), accuracy, recall, specificity,
    significance_ratio, n_pos, n_neg.  `positive[i] != 0` marks the class counted as 1 (disease for
    training_class == 'nm', group_analysis_1x1.py:118-121)."""
    dev = require_gpu(device)
    if len(scores) != len(positive):
        raise ValueError("scores and positive must have the same number of sets")
    s, off, sizes = _segments(scores, dev, torch.float32)
    l, _, sizes_l = _segments(positive, dev, torch.int32)
    if sizes != sizes_l:
        raise ValueError("every score set needs one label per score")
    if max(sizes) > _lib.NM_METRICS_MAX_N:
        raise ValueError(f"at most {_lib.NM_METRICS_MAX_N} scores per set, got {max(sizes)}")
    out = torch.empty(len(sizes), _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    thr = None
    if thresholds is not None:
        thr = torch.tensor([float(t) for t in thresholds], dtype=torch.float64, device=dev)
        if thr.numel() != len(sizes):
            raise ValueError("one threshold per set")
    _lib.check(_lib.load().nm_posthoc_metrics(s.data_ptr(), l.data_ptr(), off.data_ptr(), len(sizes), max(max(sizes), 1),
                                               thr.data_ptr() if thr is not None else None, out.data_ptr(),
                                               _stream_ptr(dev)), "nm_posthoc_metrics")
    return out


def confusion_metrics(pred: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], device="cuda:0") -> torch.Tensor:
    """One row per set: accuracy, auroc, sensitivity, specificity, f1_score, precision, n_pos, n_neg."""
    dev = require_gpu(device)
    p, off, sizes = _segments(pred, dev, torch.int32)
    l, _, sizes_l = _segments(labels, dev, torch.int32)
    if sizes != sizes_l:
        raise ValueError("every prediction needs one label")
    out = torch.empty(len(sizes), _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().nm_confusion_metrics(p.data_ptr(), l.data_ptr(), off.data_ptr(), len(sizes), out.data_ptr(),
                                                 _stream_ptr(dev)), "nm_confusion_metrics")
    return out


def _to_dev(table, dev):
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)


def _max_rows(mats):
    return max(max(int(m.shape[0]) for m in mats), 1)


def _set_table(struct, mats: Sequence[torch.Tensor], **fields):
    """The pointer table of any of the table entry points on the host, `struct` one of _lib.NmRoiSet / NmRegSet / NmNormSet:
    every matrix where it lies (x = data_ptr of the view, its row stride as pitch), and where the struct has row_off the sum of
    the heights before the set (where its per-row outputs start).  fields: the struct's other members by name -- a pointer
    member takes one tensor (or None) per set, a *pitch member an int for all sets or one tensor per set (its row stride).  A
    set without rows keeps null pointers and zero pitches of its own; a field given as None stays zero."""
    table = (struct * len(mats))()
    sets = list(table)                                            # (views of the entries, made once)
    rows = [int(m.shape[0]) for m in mats]
    for e, m, n in zip(sets, mats, rows):
        e.rows, e.pitch = n, (int(m.stride(0)) if n > 1 else int(m.shape[1]))
        if n:
            e.x = m.data_ptr()
    if hasattr(struct, "row_off"):
        off = 0
        for e, n in zip(sets, rows):
            e.row_off = off
            off += n
    for name, v in fields.items():
        if v is None:
            continue
        if isinstance(v, int):
            for e in sets:
                setattr(e, name, v)
        elif name.endswith("pitch"):
            for e, b, n in zip(sets, v, rows):
                if n and b is not None:
                    setattr(e, name, int(b.stride(0)) if n > 1 else int(b.shape[1]))
        else:
            for e, b, n in zip(sets, v, rows):
                if n and b is not None:
                    setattr(e, name, b.data_ptr())
    return table


def _roi_table(mats, groups):
    return _set_table(_lib.NmRoiSet, mats, group=groups)


def _reg_table(mats, targets, covs, incs, n_cov: int):
    return _set_table(_lib.NmRegSet, mats, target=targets, cov=covs if n_cov else None, include=incs, cov_pitch=n_cov)


def _norm_table(mats, groups=None, subs=None, zs=None):
    return _set_table(_lib.NmNormSet, mats, group=groups, sub=subs, sub_pitch=subs, z=zs, z_pitch=zs)


def _fit_table(mats, locs, groups, var=None, col_var=None):
    return _set_table(_lib.NmFitSet, mats, loc=locs, loc_pitch=locs, var=var, var_pitch=var, col_var=col_var, group=groups)


def _table_check(mats: Sequence[torch.Tensor], per_row: Optional[Sequence] = None) -> int:
    """The argument checks every table entry point's host function shares (no device is looked for): a list of [n_k, D] fp32
    tables with unit column stride and, where given, one per-row sequence (group words, targets) per table; D."""
    if len(mats) == 0:
        raise ValueError("no ROI tables")
    if per_row is not None and len(mats) != len(per_row):
        raise ValueError("mats and groups must have the same number of sets")
    D = None
    for k, m in enumerate(mats):
        if not isinstance(m, torch.Tensor) or m.dim() != 2 or m.dtype != torch.float32:
            raise ValueError(f"set {k}: a 2-D float32 tensor is needed")
        n, d = int(m.shape[0]), int(m.shape[1])
        if D is None:
            D = d
        if d != D or D < 1:
            raise ValueError(f"set {k}: {d} columns, every set needs the same number (>= 1; set 0 has {D})")
        if n > _lib.NM_METRICS_MAX_N:
            raise ValueError(f"set {k}: at most {_lib.NM_METRICS_MAX_N} rows per set, got {n}")
        if n > 0 and m.stride(1) != 1:
            raise ValueError(f"set {k}: columns must be contiguous (stride(1) == 1), got {m.stride(1)}")
        if n > 1 and m.stride(0) < D:
            raise ValueError(f"set {k}: row stride {m.stride(0)} below the {D} columns")
        if per_row is not None and int(torch.as_tensor(per_row[k]).numel()) != n:
            raise ValueError(f"set {k}: one group entry per row is needed")
    return D


def _table_device(mats: Sequence[torch.Tensor], device):
    """The device of checked tables (`device`, else where the first one lies); every table must lie on it."""
    dev = require_gpu(device if device is not None else (mats[0].device if mats[0].is_cuda else None))
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    for k, m in enumerate(mats):
        if m.device != dev:
            raise ValueError(f"set {k} is on {m.device}, not on {dev}: the tables are read where they lie")
    return dev


def _row_words(seqs: Sequence, dev, dtype, nonzero: bool = False):
    """Per-row sequences (int32 group / include words, fp32 targets) on the device, one 1-D tensor per set; a None entry stays
    None.  Host entries of all sets go up in one copy and come back as views of it (a copy per set costs more than the kernels at
    256 sets); a single entry, or any with one already on the device, is used or moved where it lies.  nonzero: the words
    become 0 / 1 (entry != 0).  A pointer table holds their addresses only: the caller keeps the list until its launch is queued."""
    parts = [None if s is None else torch.as_tensor(s).reshape(-1) for s in seqs]
    if nonzero:
        parts = [None if p is None else p.ne(0) for p in parts]
    have = [p for p in parts if p is not None]
    if len(have) < 2 or any(p.is_cuda for p in have):
        return [None if p is None else p.to(device=dev, dtype=dtype).contiguous() for p in parts]
    views = iter(torch.split(torch.cat([p.to(dtype) for p in have]).to(dev), [int(p.numel()) for p in have]))
    return [None if p is None else next(views) for p in parts]


def _seed_check(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an unsigned 64-bit integer, got {seed}")
    return seed


def _host_f32(v) -> torch.Tensor:
    """A tensor or array-like as a host fp32 tensor."""
    return torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float32))


def roi_effect(mats: Sequence[torch.Tensor], groups: Sequence, device=None) -> torch.Tensor:
    """[n_sets, D, 8] fp64 on the device, per (set, ROI column): cliff_delta, auc, n_more, n_less, n_x, n_y, mean_x, mean_y
    (ROI_EFFECT_COLUMNS; include/nmhip.h has the definitions).  mats[k]: a [n_k, D] fp32 device tensor of any row stride
    and unit column stride -- a view such as job.out_sqerr[m][:n] is read where it lies; groups[k]: n_k entries, 1 = X
    (the patients), 0 = Y (the controls), any other value leaves the row out.  One launch for all sets."""
    D = _table_check(mats, groups)
    dev = _table_device(mats, device)
    grp = _row_words(groups, dev, torch.int32)                  # (held until the launch is queued: the table holds pointers only)
    sets = _to_dev(_roi_table(mats, grp), dev)
    out = torch.empty(len(mats), D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().nm_roi_effect(sets.data_ptr(), len(mats), D, _max_rows(mats), out.data_ptr(), _stream_ptr(dev)),
               "nm_roi_effect")
    return out


# nm_roi_significance's workspace above this many bytes: the sets run in consecutive groups that fit
ROI_SIGNIFICANCE_WORKSPACE_CAP = 1 << 30


ROI_SIGNIFICANCE_MAX_D = 8192


def _perm_args(n_perm, seed):
    n_perm = int(n_perm)
    if not 0 <= n_perm <= _lib.NM_ROI_MAX_PERM:
        raise ValueError(f"n_perm must lie in 0..{_lib.NM_ROI_MAX_PERM}, got {n_perm}")
    return n_perm, _seed_check(seed)


def roi_significance(mats: Sequence[torch.Tensor], groups: Sequence, n_perm: int = 0, seed: int = 0, device=None,
                     return_maxstat: bool = False):
    """[n_sets, D, 8] fp64 on the device, per (set, ROI column): u_x, tie_term, z, p_mwu, q_bh, p_perm, p_maxt, n_perm
    (ROI_SIGNIFICANCE_COLUMNS; include/nmhip.h has the definitions): the Mann-Whitney U of X with its tie-corrected,
    continuity-corrected asymptotic two-sided p, the Benjamini-Hochberg q over the set's valid columns, and with n_perm > 0
    (at most NM_ROI_MAX_PERM) the label-permutation p-values of |S| per column and against the maximum over the columns
    (family-wise error control over the ROIs).  mats and groups as for roi_effect; a column with a NaN in an included row,
    and every column of a set with an empty group, is NaN throughout.  return_maxstat: also the [n_sets, n_perm] int32
    null distribution of the maximum (-1 for a set without a valid column).

    The rows of a set are taken as independent observations: a cohort recipe that repeats a subject across folds makes the
    p-values of the pooled rows too small.

    The workspace comes from nm_roi_significance_workspace; above ROI_SIGNIFICANCE_WORKSPACE_CAP the sets run in
    consecutive groups of a power of two that fit, set k keeping its own index in the permutation hash (the group's
    offset goes into the seed, as include/nmhip.h describes).  The same seed gives the same bytes."""
    D = _table_check(mats, groups)
    n_perm, seed = _perm_args(n_perm, seed)
    if D > ROI_SIGNIFICANCE_MAX_D:
        raise ValueError(f"at most {ROI_SIGNIFICANCE_MAX_D} columns (the Benjamini-Hochberg sort's limit), got {D}")
    dev = _table_device(mats, device)
    grp = _row_words(groups, dev, torch.int32)
    table = bytes(_roi_table(mats, grp))
    lib, n_sets, entry, max_rows = _lib.load(), len(mats), C.sizeof(_lib.NmRoiSet), _max_rows(mats)
    per = 1 << (n_sets - 1).bit_length()                   # sets per launch: the largest power of two whose workspace fits
    while per > 1 and lib.nm_roi_significance_workspace(min(per, n_sets), D, max_rows, n_perm) > ROI_SIGNIFICANCE_WORKSPACE_CAP:
        per >>= 1
    need = int(lib.nm_roi_significance_workspace(min(per, n_sets), D, max_rows, n_perm))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(n_sets, D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    maxstat = torch.empty(n_sets, n_perm, dtype=torch.int32, device=dev) if return_maxstat else None
    for k0 in range(0, n_sets, per):
        k1 = min(k0 + per, n_sets)
        sets = _to_dev(table[k0 * entry:k1 * entry], dev)
        _lib.check(lib.nm_roi_significance(sets.data_ptr(), k1 - k0, D, max_rows, n_perm, seed ^ ((k0 << 40) & ((1 << 64) - 1)),
                                           ws.data_ptr(), need, out[k0:k1].data_ptr(),
                                           maxstat[k0:k1].data_ptr() if maxstat is not None and n_perm else None,
                                           _stream_ptr(dev)), "nm_roi_significance")
    return (out, maxstat) if return_maxstat else out


def _two_groups(X, Y):
    """X over Y as one fp32 [n, D] host matrix with its group words, and whether the inputs were 1-D."""
    x, y = _host_f32(X), _host_f32(Y)
    if x.dim() != y.dim() or x.dim() not in (1, 2) or (x.dim() == 2 and x.shape[1] != y.shape[1]):
        raise ValueError(f"X and Y must both be 1-D, or 2-D with the same columns; got {tuple(x.shape)} and {tuple(y.shape)}")
    both = torch.cat([x.reshape(len(x), -1), y.reshape(len(y), -1)])
    if both.shape[0] > _lib.NM_METRICS_MAX_N:
        raise ValueError(f"at most {_lib.NM_METRICS_MAX_N} observations in X and Y together, got {both.shape[0]}")
    group = torch.cat([torch.ones(len(x), dtype=torch.int32), torch.zeros(len(y), dtype=torch.int32)])
    return both, group, x.dim() == 1


def mann_whitney(X, Y, n_perm: int = 0, seed: int = 0, device=None):
    """scipy.stats.mannwhitneyu(X, Y, alternative='two-sided', method='asymptotic', use_continuity=True) on the device, with
    the Benjamini-Hochberg q over the columns and (n_perm > 0) the permutation p-values of roi_significance: a dict of
    ROI_SIGNIFICANCE_COLUMNS -- floats for 1-D inputs, [D] numpy arrays for [n, D] inputs (one test per column).
    len(X) + len(Y) <= NM_METRICS_MAX_N; the observations are taken as independent."""
    both, group, flat = _two_groups(X, Y)
    n_perm, seed = _perm_args(n_perm, seed)
    dev = require_gpu(device)
    tab = roi_significance([both.to(dev)], [group], n_perm=n_perm, seed=seed, device=dev)[0].cpu().numpy()
    return {name: (float(tab[0, j]) if flat else tab[:, j].copy()) for j, name in enumerate(ROI_SIGNIFICANCE_COLUMNS)}


def cliff_delta(X, Y, device=None):
    """cliff_delta(X, Y) of utils.py:97-109 on the device: 1-D inputs give a float, [n, D] inputs a [D] numpy array (one
    delta per column).  len(X) + len(Y) <= NM_METRICS_MAX_N."""
    both, group, flat = _two_groups(X, Y)
    dev = require_gpu(device)
    delta = roi_effect([both.to(dev)], [group], device=dev)[0, :, 0].cpu().numpy()
    return float(delta[0]) if flat else delta


AUC_BOOTSTRAP_COLUMNS = ("roc_auc", "ci_lo", "ci_hi", "boot_mean", "boot_se", "n_boot", "n_pos", "n_neg")
AUC_COMPARE_COLUMNS = ("delta_auc", "ci_lo", "ci_hi", "boot_mean", "boot_se", "p_boot", "n_le0", "n_ge0")
AUC_BOOTSTRAP_MAX_STREAM = (1 << 24) - 1


def boot_indices(n_boot: int, ci: float):
    """The two order statistics of a `ci` interval over n_boot resamples: lo = floor((1 - ci) / 2 * (n_boot - 1)) and
    hi = n_boot - 1 - lo -- np.quantile's method='lower' at (1 - ci) / 2 and method='higher' at (1 + ci) / 2."""
    lo = int(np.floor((1.0 - ci) / 2.0 * (n_boot - 1)))
    return lo, n_boot - 1 - lo


def _boot_check(scores, positive, n_boot, ci, seed, streams, pairs):
    """nm_auc_bootstrap's argument checks on the host (no device is looked for): the sizes, n_boot, the two indices, the
    seed, the stream ids and the pairs as host values."""
    if len(scores) == 0:
        raise ValueError("no score sets")
    if len(scores) != len(positive):
        raise ValueError("scores and positive must have the same number of sets")
    sizes = [int(torch.as_tensor(s).numel()) for s in scores]
    if sizes != [int(torch.as_tensor(p).numel()) for p in positive]:
        raise ValueError("every score set needs one label per score")
    if max(sizes) > _lib.NM_METRICS_MAX_N:
        raise ValueError(f"at most {_lib.NM_METRICS_MAX_N} scores per set, got {max(sizes)}")
    n_boot, ci = int(n_boot), float(ci)
    if not 1 <= n_boot <= _lib.NM_BOOT_MAX:
        raise ValueError(f"n_boot must lie in 1..{_lib.NM_BOOT_MAX}, got {n_boot}")
    if not 0.0 < ci < 1.0:
        raise ValueError(f"ci must lie in (0, 1), got {ci}")
    seed = _seed_check(seed)
    if streams is not None:
        streams = [int(v) for v in np.asarray(streams).reshape(-1)]
        if len(streams) != len(sizes):
            raise ValueError("one stream id per set")
        if any(not 0 <= v <= AUC_BOOTSTRAP_MAX_STREAM for v in streams):
            raise ValueError(f"stream ids must lie in 0..{AUC_BOOTSTRAP_MAX_STREAM}")
    elif len(sizes) - 1 > AUC_BOOTSTRAP_MAX_STREAM:
        raise ValueError(f"more than {AUC_BOOTSTRAP_MAX_STREAM + 1} sets need explicit stream ids")
    if pairs is not None:
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2) if len(pairs) else np.zeros((0, 2), dtype=np.int64)
        if pairs.size and (pairs.min() < 0 or pairs.max() >= len(sizes)):
            raise ValueError(f"pair indices must lie in 0..{len(sizes) - 1}")
    lo, hi = boot_indices(n_boot, ci)
    return sizes, n_boot, lo, hi, seed, streams, pairs


def auc_bootstrap(scores: Sequence[torch.Tensor], positive: Sequence[torch.Tensor], n_boot: int = 2000, ci: float = 0.95,
                  seed: int = 0, streams=None, pairs=None, device="cuda:0", return_boot: bool = False):
    """[n_sets, 8] fp64 on the device, per set: roc_auc, ci_lo, ci_hi, boot_mean, boot_se, n_boot, n_pos, n_neg
    (AUC_BOOTSTRAP_COLUMNS; include/nmhip.h has the definitions): the set's ROC-AUC with the percentile interval, mean and
    standard error of n_boot stratified bootstrap resamples (positives and negatives are redrawn within their class, as
    pROC does by default).  scores / positive as for posthoc_metrics.  streams[k] (default k, 0..2^24 - 1) names set k's
    random stream: sets with the same stream id and the same labels draw the same subjects in every resample.  pairs: a list
    of set index pairs (a, c); then also [n_pairs, 8] fp64 = delta_auc, ci_lo, ci_hi, boot_mean, boot_se, p_boot, n_le0,
    n_ge0 (AUC_COMPARE_COLUMNS) of the resamples' differences AUC_a - AUC_c -- NaN unless the two sets share the stream id
    and the labels.  return_boot: also the [n_sets, n_boot] int32 distribution of A2* = AUC* x 2 n_pos n_neg (-1 for a
    set that is not valid: one class only, a NaN score, an empty set).

    The rows of a set are taken as independent subjects: a cohort recipe that repeats a subject across folds makes the
    interval of the pooled rows too narrow.  The same seed gives the same bytes."""
    sizes, n_boot, lo, hi, seed, streams, pairs = _boot_check(scores, positive, n_boot, ci, seed, streams, pairs)
    dev = require_gpu(device)
    s, off, _ = _segments([torch.as_tensor(p) for p in scores], dev, torch.float32)
    l, _, _ = _segments([torch.as_tensor(p) for p in positive], dev, torch.int32)
    n_sets, max_set = len(sizes), max(max(sizes), 1)
    n_pairs = 0 if pairs is None else int(pairs.shape[0])
    st = torch.tensor(streams, dtype=torch.int32, device=dev) if streams is not None else None
    pr = torch.as_tensor(pairs, dtype=torch.int32).contiguous().to(dev) if n_pairs else None
    lib = _lib.load()
    need = int(lib.nm_auc_bootstrap_workspace(n_sets, max_set, n_boot, n_pairs))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(n_sets, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    pout = torch.empty(n_pairs, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev) if pairs is not None else None
    boot = torch.empty(n_sets, n_boot, dtype=torch.int32, device=dev) if return_boot else None
    _lib.check(lib.nm_auc_bootstrap(s.data_ptr(), l.data_ptr(), off.data_ptr(), st.data_ptr() if st is not None else None,
                                    n_sets, max_set, n_boot, lo, hi, seed, pr.data_ptr() if pr is not None else None, n_pairs,
                                    ws.data_ptr(), need, out.data_ptr(), pout.data_ptr() if n_pairs else None,
                                    boot.data_ptr() if boot is not None else None, _stream_ptr(dev)), "nm_auc_bootstrap")
    res = (out,) + ((pout,) if pairs is not None else ()) + ((boot,) if return_boot else ())
    return res if len(res) > 1 else out


def auc_compare(scores_a, scores_c, positive, n_boot: int = 2000, ci: float = 0.95, seed: int = 0, device="cuda:0"):
    """Two procedures' scores of the same subjects: the difference of their ROC-AUCs with its paired stratified-bootstrap
    interval and two-sided p -- a dict of AUC_COMPARE_COLUMNS (floats)."""
    a, c, p = (torch.as_tensor(v).reshape(-1) for v in (scores_a, scores_c, positive))
    if a.numel() != c.numel():
        raise ValueError(f"both procedures need the same subjects, got {a.numel()} and {c.numel()} scores")
    _, prs = auc_bootstrap([a, c], [p, p], n_boot=n_boot, ci=ci, seed=seed, streams=[0, 0], pairs=[(0, 1)], device=device)
    row = prs[0].cpu().numpy()
    return {name: float(row[j]) for j, name in enumerate(AUC_COMPARE_COLUMNS)}


OPERATING_POINT_COLUMNS = ("threshold", "accuracy", "recall", "specificity", "tp", "fp", "objective", "status")
ROC_SUMMARY_COLUMNS = ("roc_auc", "average_precision", "pauc", "sens_at_spec", "spec_at_sens", "n_thresholds", "n_pos", "n_neg")
OPERATING_RULES = {"roc": _lib.NM_OP_ROC, "f1": _lib.NM_OP_F1, "pr": _lib.NM_OP_PR, "cost": _lib.NM_OP_COST,
                   "eer": _lib.NM_OP_EER, "f1max": _lib.NM_OP_F1MAX, "spec": _lib.NM_OP_SPEC}


def _op_check(scores, positive, rules, select_of, evaluate, grid, cost_fn, cost_fp, spec, sens, max_fpr, roc_grid):
    """nm_operating_points' argument checks on the host (no device is looked for): the sizes, the rule names, the threshold
    grid, the costs, the three rates, the ROC grid and the two index lists as host values."""
    if len(scores) == 0:
        raise ValueError("no score sets")
    if len(scores) != len(positive):
        raise ValueError("scores and positive must have the same number of sets")
    sizes = [int(torch.as_tensor(s).numel()) for s in scores]
    if sizes != [int(torch.as_tensor(p).numel()) for p in positive]:
        raise ValueError("every score set needs one label per score")
    if max(sizes) > _lib.NM_METRICS_MAX_N:
        raise ValueError(f"at most {_lib.NM_METRICS_MAX_N} scores per set, got {max(sizes)}")
    rules = [rules] if isinstance(rules, str) else list(rules)
    if not 1 <= len(rules) <= _lib.NM_OP_MAX_RULES:
        raise ValueError(f"between 1 and {_lib.NM_OP_MAX_RULES} rules, got {len(rules)}")
    for r in rules:
        if r not in OPERATING_RULES:
            raise ValueError(f"rule must be one of {sorted(OPERATING_RULES)}, got {r!r}")
    if len(grid) != 3:
        raise ValueError("grid is (lo, hi, n)")
    lo, hi, n = float(grid[0]), float(grid[1]), int(grid[2])
    if n != grid[2] or not 2 <= n <= _lib.NM_OP_MAX_LINSPACE:
        raise ValueError(f"the threshold grid needs 2..{_lib.NM_OP_MAX_LINSPACE} values, got {grid[2]!r}")
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"the threshold grid's ends must be finite, got {grid[0]!r}, {grid[1]!r}")
    cost_fn, cost_fp, spec, sens, max_fpr = float(cost_fn), float(cost_fp), float(spec), float(sens), float(max_fpr)
    if not (np.isfinite(cost_fn) and np.isfinite(cost_fp)):
        raise ValueError("cost_fn and cost_fp must be finite")
    if not (0.0 <= spec <= 1.0 and 0.0 <= sens <= 1.0):
        raise ValueError(f"spec and sens must lie in [0, 1], got {spec}, {sens}")
    if not 0.0 < max_fpr <= 1.0:
        raise ValueError(f"max_fpr must lie in (0, 1], got {max_fpr}")
    roc_grid = int(roc_grid)
    if not 0 <= roc_grid <= _lib.NM_OP_MAX_GRID:
        raise ValueError(f"roc_grid must lie in 0..{_lib.NM_OP_MAX_GRID}, got {roc_grid}")
    n_sets = len(sizes)
    evaluate = list(range(n_sets)) if evaluate is None else [int(v) for v in np.asarray(evaluate).reshape(-1)]
    select_of = list(evaluate) if select_of is None else [int(v) for v in np.asarray(select_of).reshape(-1)]
    if not evaluate:
        raise ValueError("no evaluation entry")
    if len(select_of) != len(evaluate):
        raise ValueError("select_of needs one set index per evaluation entry")
    if any(not 0 <= v < n_sets for v in evaluate + select_of):
        raise ValueError(f"set indices must lie in 0..{n_sets - 1}")
    table = (_lib.NmOpRule * len(rules))()
    for k, r in enumerate(rules):
        table[k].kind, table[k].n, table[k].a, table[k].b = OPERATING_RULES[r], n, lo, hi
        table[k].cost_fn, table[k].cost_fp = cost_fn, cost_fp
        if r == "spec":
            table[k].a = spec
    return sizes, table, select_of, evaluate, spec, sens, max_fpr, roc_grid


def operating_points(scores: Sequence[torch.Tensor], positive: Sequence[torch.Tensor], rules=("roc",), select_of=None,
                     evaluate=None, grid=(0.0, 1.0, 100), cost_fn: float = 1.0, cost_fp: float = 1.0, spec: float = 0.9,
                     sens: float = 0.9, max_fpr: float = 0.1, roc_grid: int = 0, device="cuda:0"):
    """(points [n_eval, n_rules, 8], summary [n_sets, 8]) fp64 on the device, and [n_sets, roc_grid] when roc_grid > 0
    (OPERATING_POINT_COLUMNS, ROC_SUMMARY_COLUMNS; include/nmhip.h has the definitions).  scores / positive as for
    posthoc_metrics.  rules: names out of OPERATING_RULES -- "roc", "f1", "pr", "cost", "eer" are the five methods of
    compute_classification_performance (group_analysis_1x1.py:105-157), "f1max" the best F1 over every distinct score, "spec"
    the lowest threshold whose specificity is at least `spec`.  Entry e scores set evaluate[e] (default: every set in order)
    with the thresholds selected on set select_of[e] (default: evaluate[e]): the reference's `optimal_threshold=` mode, a
    threshold fitted on one set of subjects and applied to another.  grid = (lo, hi, n): the np.linspace of "f1" and "cost";
    cost_fn / cost_fp: the two costs of "cost"; spec / sens: the rates of sens_at_spec / spec_at_sens; max_fpr: the partial
    AUC's limit.  status 1 marks the "pr" rule where the reference's argmax lands on a NaN (the top score is a control),
    -2 a row without a curve (NaN).  One call, two launches, for all sets; the same input gives the same bytes."""
    sizes, table, select_of, evaluate, spec, sens, max_fpr, G = _op_check(scores, positive, rules, select_of, evaluate, grid,
                                                                           cost_fn, cost_fp, spec, sens, max_fpr, roc_grid)
    dev = require_gpu(device)
    s, off, _ = _segments([torch.as_tensor(p) for p in scores], dev, torch.float32)
    l, _, _ = _segments([torch.as_tensor(p) for p in positive], dev, torch.int32)
    n_sets, n_rules, n_eval = len(sizes), len(table), len(evaluate)
    sel = torch.tensor(select_of, dtype=torch.int32, device=dev)
    ev = torch.tensor(evaluate, dtype=torch.int32, device=dev)
    lib = _lib.load()
    need = int(lib.nm_operating_points_workspace(n_sets, n_rules))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    points = torch.empty(n_eval, n_rules, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    summary = torch.empty(n_sets, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    curve = torch.empty(n_sets, G, dtype=torch.float64, device=dev) if G else None
    _lib.check(lib.nm_operating_points(s.data_ptr(), l.data_ptr(), off.data_ptr(), n_sets, max(max(sizes), 1), table, n_rules,
                                       sel.data_ptr(), n_eval, ev.data_ptr(), spec, sens, max_fpr, ws.data_ptr(), need,
                                       points.data_ptr(), summary.data_ptr(), curve.data_ptr() if G else None, G,
                                       _stream_ptr(dev)), "nm_operating_points")
    return (points, summary, curve) if G else (points, summary)


def classification_performance(scores, positive, method: str = "roc", optimal_threshold=None, device="cuda:0"):
    """compute_classification_performance of group_analysis_1x1.py:105-157 on one score set: (roc_auc, accuracy, recall,
    specificity, significance_ratio) as floats.  method: "roc", "f1", "pr", "cost" (costs 1 and 1, :138) or "eer" chooses the
    threshold on the set itself; optimal_threshold, where given, is used instead (:128)."""
    if method not in ("roc", "f1", "pr", "cost", "eer"):
        raise ValueError("Unknown method for finding optimal threshold")
    sc, po = torch.as_tensor(scores).reshape(-1), torch.as_tensor(positive).reshape(-1)
    if optimal_threshold is not None:
        row = posthoc_metrics([sc], [po], thresholds=[float(optimal_threshold)], device=device)[0].cpu().numpy()
        return tuple(float(row[j]) for j in (0, 2, 3, 4, 5))
    points, summary = operating_points([sc], [po], rules=(method,), device=device)
    row, auc = points[0, 0].cpu().numpy(), float(summary[0, 0])
    return auc, float(row[1]), float(row[2]), float(row[3]), auc / (1.0 - auc)


def _reg_check(mats, targets, kind, covariates, include):
    """nm_column_regress's argument checks on the host (no device is looked for): D, the kind's code, n_cov."""
    if kind not in COLUMN_REGRESS_KINDS:
        raise ValueError(f"kind must be one of {sorted(COLUMN_REGRESS_KINDS)}, got {kind!r}")
    D = _table_check(mats, targets)                         # (one target entry per row)
    for name, seq in (("covariates", covariates), ("include", include)):
        if seq is not None and len(seq) != len(mats):
            raise ValueError(f"{name} must have one entry per set")
    n_cov = 0
    if covariates is not None:
        for k, c in enumerate(covariates):
            c = torch.as_tensor(c)
            if c.dim() != 2 or int(c.shape[0]) != int(mats[k].shape[0]):
                raise ValueError(f"set {k}: covariates must be [rows, q], got {tuple(c.shape)}")
            if k == 0:
                n_cov = int(c.shape[1])
            if int(c.shape[1]) != n_cov:
                raise ValueError(f"set {k}: {int(c.shape[1])} covariates, every set needs the same number (set 0 has {n_cov})")
        if n_cov > _lib.NM_REG_MAX_COV:
            raise ValueError(f"at most {_lib.NM_REG_MAX_COV} covariates, got {n_cov}")
    if include is not None:
        for k, w in enumerate(include):
            if w is not None and int(torch.as_tensor(w).numel()) != int(mats[k].shape[0]):
                raise ValueError(f"set {k}: one include word per row is needed")
    return D, COLUMN_REGRESS_KINDS[kind], n_cov


def column_regress(mats: Sequence[torch.Tensor], targets: Sequence, kind: str = "ols", covariates: Optional[Sequence] = None,
                   include: Optional[Sequence] = None, device=None) -> torch.Tensor:
    """[n_sets, D, 8] fp64 on the device, per (set, column): const, coef, se_const, se_coef, p_const, p_coef, n_obs, n_iter
    (COLUMN_REGRESS_COLUMNS; include/nmhip.h has the definitions): the fit target ~ const + column + covariates, "ols" (least
    squares, Student-t p-values) or "logit" (maximum likelihood by Newton steps, Wald p-values), one fit per column.
    mats[k]: a [n_k, D] fp32 device tensor read where it lies, as for roi_effect; targets[k]: n_k values (0 / 1 for logit);
    covariates[k]: [n_k, q] nuisance regressors, q <= NM_REG_MAX_COV, whose coefficients are not reported; include[k]: n_k
    words (or None), a row with 0 is left out and never looked at.  n_iter < 0 is a status with NaN statistics: -1 a Logit
    that did not converge (perfect separation ends here), -2 invalid input.  One launch for all sets."""
    D, code, n_cov = _reg_check(mats, targets, kind, covariates, include)
    dev = _table_device(mats, device)
    tgt = _row_words(targets, dev, torch.float32)
    cov = [torch.as_tensor(c).to(device=dev, dtype=torch.float32).contiguous() for c in covariates] if n_cov else None
    inc = _row_words(include, dev, torch.int32, nonzero=True) if include is not None else None
    sets = _to_dev(_reg_table(mats, tgt, cov, inc, n_cov), dev)
    out = torch.empty(len(mats), D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().nm_column_regress(sets.data_ptr(), len(mats), D, _max_rows(mats), n_cov, code, out.data_ptr(),
                                              _stream_ptr(dev)), "nm_column_regress")
    return out


def latent_pvalues(latent, target, type, device=None):
    """latent_pvalues(latent, target, type) of utils_vae.py:163-174 on the device: a DataFrame with labels = ['const',
    'latent'] and one column 'latent i' per latent dimension holding the p-values of target ~ const + latent_i;
    type == 'continuous' is OLS, anything else Logit.  A fit that statsmodels would refuse (separation, a constant
    column) gives NaN."""
    lat, tgt = _host_f32(latent), _host_f32(target)
    if lat.dim() != 2 or tgt.dim() != 1 or tgt.numel() != lat.shape[0]:
        raise ValueError(f"latent must be [n, Z] and target [n]; got {tuple(lat.shape)} and {tuple(tgt.shape)}")
    _reg_check([lat], [tgt], "ols", None, None)
    dev = require_gpu(device)
    tab = column_regress([lat.to(dev)], [tgt], kind="ols" if type == "continuous" else "logit", device=dev)[0].cpu().numpy()
    from .io import latent_pvalues_frame
    return latent_pvalues_frame(tab)


COHORT_MOMENTS_COLUMNS = ("mean", "sd", "var", "n_ref", "min", "max", "n_nonfinite", "status")
NORMATIVE_ROW_COLUMNS = ("n_hi", "n_lo", "mean_z", "mean_abs_z", "max_z", "argmax_z", "n_valid", "status")
NORMATIVE_COL_COLUMNS = ("n_hi_x", "n_lo_x", "n_hi_y", "n_lo_y", "n_x", "n_y", "mean_z_x", "mean_z_y")


def _norm_check(mats, groups, sub) -> int:
    """_table_check, and a `sub` matrix of the same shape and kind per set (no device is looked for); the width."""
    D = _table_check(mats, groups)
    if sub is not None:
        if len(sub) != len(mats):
            raise ValueError("sub must have one entry per set")
        for k, (m, b) in enumerate(zip(mats, sub)):
            if not isinstance(b, torch.Tensor) or b.dtype != torch.float32 or b.shape != m.shape:
                raise ValueError(f"set {k}: sub must be a float32 tensor of the table's shape {tuple(m.shape)}")
            if b.shape[0] > 0 and b.stride(1) != 1:
                raise ValueError(f"set {k}: the columns of sub must be contiguous")
            if b.device != m.device:
                raise ValueError(f"set {k}: sub is on {b.device}, the table on {m.device}")
    return D


def _ref_check(ref_of, n_sets, n_ref, lowest: int = 0):
    """ref_of as a list of ints inside lowest..n_ref-1 (None: set k takes row k, so n_sets <= n_ref); lowest = -1 where an
    entry point reads -1 as "no reference"."""
    if ref_of is None:
        if n_sets > n_ref:
            raise ValueError(f"{n_sets} sets but {n_ref} reference entries: ref_of is needed")
        return None
    ref = [int(v) for v in np.asarray(ref_of).reshape(-1)]
    if len(ref) != n_sets:
        raise ValueError("ref_of must have one entry per set")
    if any(not lowest <= v < n_ref for v in ref):
        raise ValueError(f"ref_of entries must lie in {lowest}..{n_ref - 1}")
    return ref


def cohort_moments(mats: Sequence[torch.Tensor], groups: Sequence, sub: Optional[Sequence[torch.Tensor]] = None, ddof: int = 1,
                   device=None) -> torch.Tensor:
    """[n_sets, D, 8] fp64 on the device, per (set, column) over the rows whose group word is 0 (the reference cohort): mean,
    sd, var, n_ref, min, max, n_nonfinite, status (COHORT_MOMENTS_COLUMNS; include/nmhip.h has the definitions).  mats /
    groups as for roi_effect; sub[k] (optional, the shape of mats[k]): the value is mats[k] - sub[k] in fp64 (a table against
    its out_loc export: the signed residual).  status -2 (mean, sd, var NaN): n_ref <= ddof, a non-finite reference value, a
    constant column.  One launch for all sets."""
    if ddof not in (0, 1) or isinstance(ddof, bool):
        raise ValueError(f"ddof must be 0 or 1, got {ddof!r}")
    D = _norm_check(mats, groups, sub)
    dev = _table_device(mats, device)
    grp = _row_words(groups, dev, torch.int32)
    sets = _to_dev(_norm_table(mats, grp, sub), dev)
    out = torch.empty(len(mats), D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().nm_cohort_moments(sets.data_ptr(), len(mats), D, _max_rows(mats), int(ddof), out.data_ptr(),
                                              _stream_ptr(dev)), "nm_cohort_moments")
    return out


def normative_z(mats: Sequence[torch.Tensor], groups: Sequence, moments: torch.Tensor, ref_of=None, thr: float = 1.96,
                sub: Optional[Sequence[torch.Tensor]] = None, return_z: bool = True, device=None):
    """Every row of every set z-scored, column by column, against row ref_of[k] (default k) of a cohort_moments table:
    (z, rows, cols).  z: a list of [n_k, D] fp32 device tensors (None without return_z), NaN where the value is not finite or
    the column's moments are not valid; rows [sum n_k, 8] fp64 = n_hi, n_lo, mean_z, mean_abs_z, max_z, argmax_z, n_valid,
    status per subject (NORMATIVE_ROW_COLUMNS; n_hi counts z > thr, n_lo z < -thr), the sets one after another; cols
    [n_sets, D, 8] fp64 = n_hi_x, n_lo_x, n_hi_y, n_lo_y, n_x, n_y, mean_z_x, mean_z_y per column (NORMATIVE_COL_COLUMNS; x =
    group 1, y = group 0: the extreme-deviation map).  A row of any group is scored.  One launch pair for all sets."""
    thr = float(thr)
    if not (np.isfinite(thr) and thr > 0.0):
        raise ValueError(f"thr must be finite and > 0, got {thr}")
    D = _norm_check(mats, groups, sub)
    if D > _lib.NM_NORM_MAX_D:
        raise ValueError(f"at most {_lib.NM_NORM_MAX_D} columns, got {D}")
    if not isinstance(moments, torch.Tensor) or moments.dtype != torch.float64 or moments.dim() != 3 or \
            tuple(moments.shape[1:]) != (D, _lib.NM_METRICS_STRIDE):
        raise ValueError(f"moments must be a float64 [n, {D}, {_lib.NM_METRICS_STRIDE}] tensor as cohort_moments returns it")
    ref = _ref_check(ref_of, len(mats), int(moments.shape[0]))
    dev = _table_device(mats, device)
    grp = _row_words(groups, dev, torch.int32)
    mom = moments.to(dev).contiguous()
    zs = [torch.empty(int(m.shape[0]), D, dtype=torch.float32, device=dev) for m in mats] if return_z else None
    sets = _to_dev(_norm_table(mats, grp, sub, zs), dev)
    total = sum(int(m.shape[0]) for m in mats)
    rows = torch.empty(total, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    cols = torch.empty(len(mats), D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    rf = torch.tensor(ref, dtype=torch.int32, device=dev) if ref is not None else None
    _lib.check(_lib.load().nm_normative_z(sets.data_ptr(), len(mats), D, _max_rows(mats), mom.data_ptr(), int(mom.shape[0]),
                                           rf.data_ptr() if rf is not None else None, thr, rows.data_ptr(), cols.data_ptr(),
                                           _stream_ptr(dev)), "nm_normative_z")
    return zs, rows, cols


def _latent_width(Z: int):
    if not 1 <= Z <= _lib.NM_WIDE_MAX_LATENT:
        raise ValueError(f"the width must lie in 1..{_lib.NM_WIDE_MAX_LATENT}, got {Z}")


def cohort_cov(mats: Sequence[torch.Tensor], groups: Sequence, ridge: float = 0.0, device=None):
    """(mean [n_sets, Z], chol [n_sets, Z, Z], status [n_sets] int32) on the device, per set over the rows whose group word is
    0: the column means, and the lower Cholesky factor of their sample covariance (np.cov(rowvar=False)) plus `ridge` on the
    diagonal.  status -2 (a NaN factor): fewer than two reference rows, a non-finite value, n_ref <= Z with ridge == 0, or a
    covariance that is numerically singular.  1 <= Z <= NM_WIDE_MAX_LATENT.  One launch for all sets."""
    ridge = float(ridge)
    if not (np.isfinite(ridge) and ridge >= 0.0):
        raise ValueError(f"ridge must be finite and >= 0, got {ridge}")
    Z = _norm_check(mats, groups, None)
    _latent_width(Z)
    dev = _table_device(mats, device)
    grp = _row_words(groups, dev, torch.int32)
    sets = _to_dev(_norm_table(mats, grp), dev)
    mean = torch.empty(len(mats), Z, dtype=torch.float64, device=dev)
    chol = torch.empty(len(mats), Z, Z, dtype=torch.float64, device=dev)
    status = torch.empty(len(mats), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().nm_cohort_cov(sets.data_ptr(), len(mats), Z, _max_rows(mats), ridge, mean.data_ptr(), chol.data_ptr(),
                                          status.data_ptr(), _stream_ptr(dev)), "nm_cohort_cov")
    return mean, chol, status


def mahalanobis(mats: Sequence[torch.Tensor], mean: torch.Tensor, chol: torch.Tensor, status: torch.Tensor, ref_of=None,
                device=None):
    """A list of [n_k] fp64 device tensors: the Mahalanobis distance d = |L^-1 (row - mean)| of every row of set k to cohort
    ref_of[k] (default k) of a cohort_cov result.  NaN for a row with a non-finite entry and for every row scored against a
    factor whose status is not 0.  One launch for all sets."""
    Z = _table_check(mats)
    _latent_width(Z)
    for name, v, dt in (("mean", mean, torch.float64), ("chol", chol, torch.float64), ("status", status, torch.int32)):
        if not isinstance(v, torch.Tensor) or v.dtype != dt:
            raise ValueError(f"{name} must be a {dt} tensor as cohort_cov returns it")
    n = int(status.numel())
    if n < 1 or tuple(mean.shape) != (n, Z) or tuple(chol.shape) != (n, Z, Z) or status.dim() != 1:
        raise ValueError(f"mean [n, {Z}], chol [n, {Z}, {Z}] and status [n] are needed, got {tuple(mean.shape)}, "
                         f"{tuple(chol.shape)}, {tuple(status.shape)}")
    ref = _ref_check(ref_of, len(mats), n)
    dev = _table_device(mats, device)
    sets = _to_dev(_norm_table(mats), dev)
    total = sum(int(m.shape[0]) for m in mats)
    d2 = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
    d = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
    rf = torch.tensor(ref, dtype=torch.int32, device=dev) if ref is not None else None
    mean, chol, status = mean.to(dev).contiguous(), chol.to(dev).contiguous(), status.to(dev).contiguous()
    _lib.check(_lib.load().nm_mahalanobis(sets.data_ptr(), len(mats), Z, _max_rows(mats), mean.data_ptr(), chol.data_ptr(),
                                           status.data_ptr(), n, rf.data_ptr() if rf is not None else None, d2.data_ptr(),
                                           d.data_ptr(), _stream_ptr(dev)), "nm_mahalanobis")
    return list(torch.split(d[:total], [int(m.shape[0]) for m in mats]))


COHORT_QUANTILE_COLUMNS = ("median", "mad", "q1", "q3", "iqr", "n_ref", "n_nonfinite", "status")
CENTILE_ROW_COLUMNS = ("n_hi", "n_lo", "mean_pct", "mean_abs_dev", "max_pct", "argmax_pct", "n_valid", "status")
CENTILE_COL_COLUMNS = ("n_hi_x", "n_lo_x", "n_hi_y", "n_lo_y", "n_x", "n_y", "mean_pct_x", "mean_pct_y")
# nm_normative_centile's workspace above this many bytes: the scored sets run in consecutive groups that fit
NORMATIVE_CENTILE_WORKSPACE_CAP = 1 << 30


def _probs_check(probs):
    """The probabilities of cohort_quantiles as a list of floats: at most NM_CENT_MAX_Q, each inside [0, 1]."""
    p = [float(v) for v in np.asarray(probs, dtype=np.float64).reshape(-1)]
    if len(p) > _lib.NM_CENT_MAX_Q:
        raise ValueError(f"at most {_lib.NM_CENT_MAX_Q} probabilities, got {len(p)}")
    if any(not 0.0 <= v <= 1.0 for v in p):
        raise ValueError(f"every probability must lie in [0, 1], got {p}")
    return p


def _tail_check(tail) -> float:
    tail = float(tail)
    if not (np.isfinite(tail) and 0.0 < tail < 50.0):
        raise ValueError(f"tail must lie inside (0, 50) percent, got {tail}")
    return tail


def _centile_ref_check(ref_of, n_sets):
    """ref_of of normative_centile as a list of ints inside -1..n_sets-1 (None: every set is its own reference)."""
    if ref_of is None:
        return list(range(n_sets))
    ref = [int(v) for v in np.asarray(ref_of).reshape(-1)]
    if len(ref) != n_sets:
        raise ValueError("ref_of must have one entry per set")
    if any(not -1 <= v < n_sets for v in ref):
        raise ValueError(f"ref_of entries must lie in -1..{n_sets - 1}")
    return ref


def cohort_quantiles(mats: Sequence[torch.Tensor], groups: Sequence, probs=(0.05, 0.25, 0.5, 0.75, 0.95),
                     sub: Optional[Sequence[torch.Tensor]] = None, device=None):
    """(q [n_sets, D, n_q], stats [n_sets, D, 8]) fp64 on the device, per (set, column) over the rows whose group word is 0 (the
    reference cohort): the quantiles at `probs` (np.quantile, method="linear": the normative range, the centile curve) and
    median, mad, q1, q3, iqr, n_ref, n_nonfinite, status (COHORT_QUANTILE_COLUMNS; include/nmhip.h has the definitions; mad is
    scipy's median_abs_deviation with scale 1).  mats / groups / sub as for cohort_moments.  status -2 (everything else NaN):
    no reference row, or a non-finite reference value.  One launch for all sets."""
    p = _probs_check(probs)
    D = _norm_check(mats, groups, sub)
    dev = _table_device(mats, device)
    grp = _row_words(groups, dev, torch.int32)
    sets = _to_dev(_norm_table(mats, grp, sub), dev)
    q = torch.empty(len(mats), D, len(p), dtype=torch.float64, device=dev)
    stats = torch.empty(len(mats), D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().nm_cohort_quantiles(sets.data_ptr(), len(mats), D, _max_rows(mats), (C.c_double * max(len(p), 1))(*p),
                                                len(p), q.data_ptr() if p else None, stats.data_ptr(), _stream_ptr(dev)),
               "nm_cohort_quantiles")
    return q, stats


def _centile_groups(lib, rows, scored, D):
    """The scored sets in consecutive groups whose workspace stays below NORMATIVE_CENTILE_WORKSPACE_CAP (a set alone always runs)."""
    out, cur, n = [], [], 0
    for k in scored:
        if cur and lib.nm_normative_centile_workspace(n + rows[k], D) > NORMATIVE_CENTILE_WORKSPACE_CAP:
            out.append(cur)
            cur, n = [], 0
        cur.append(k)
        n += rows[k]
    if cur:
        out.append(cur)
    return out


def normative_centile(mats: Sequence[torch.Tensor], groups: Sequence, ref_of=None, tail: float = 2.5, loo: bool = False,
                      sub: Optional[Sequence[torch.Tensor]] = None, return_table: bool = True, device=None):
    """Every row of every scored set ranked, column by column, among the reference rows (group 0) of set ref_of[k] (default k):
    (pct, rows, cols).  ref_of[k] = -1: set k is a reference only (its pct entry is None, it owns no rows, its cols are NaN).
    pct: a list of [n_k, D] fp32 device tensors (None without return_table), the percentile rank of the value in the reference
    column (scipy's percentileofscore, kind="mean"), NaN where the value is not finite or the column has no valid reference;
    rows [sum n_k over the scored sets, 8] fp64 = n_hi, n_lo, mean_pct, mean_abs_dev, max_pct, argmax_pct, n_valid, status per
    subject (CENTILE_ROW_COLUMNS; n_hi counts pct > 100 - tail, n_lo pct < tail); cols [n_sets, D, 8] fp64 = n_hi_x, n_lo_x,
    n_hi_y, n_lo_y, n_x, n_y, mean_pct_x, mean_pct_y per column (CENTILE_COL_COLUMNS; x = group 1, y = group 0: the
    extreme-centile map).  loo: a reference row of a set that is its own reference is ranked among the other reference rows.

    The workspace comes from nm_normative_centile_workspace; above NORMATIVE_CENTILE_WORKSPACE_CAP the scored sets run in
    consecutive groups, each with the reference sets it names (as references only); the result is byte-identical."""
    tail = _tail_check(tail)
    if loo not in (False, True, 0, 1):
        raise ValueError(f"loo must be a bool, got {loo!r}")
    D = _norm_check(mats, groups, sub)
    n_sets = len(mats)
    ref = _centile_ref_check(ref_of, n_sets)
    dev = _table_device(mats, device)
    lib = _lib.load()
    grp = _row_words(groups, dev, torch.int32)
    heights = [int(m.shape[0]) for m in mats]
    scored = [k for k in range(n_sets) if ref[k] != -1]
    zs = [torch.empty(heights[k], D, dtype=torch.float32, device=dev) if ref[k] != -1 else None for k in range(n_sets)] \
        if return_table else None
    full = _norm_table(mats, grp, sub, zs)
    starts, total = {}, 0
    for k in scored:
        starts[k] = total
        total += heights[k]
    rows = torch.empty(max(total, 1), _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    plan = _centile_groups(lib, heights, scored, D)
    need = max([int(lib.nm_normative_centile_workspace(sum(heights[k] for k in g), D)) for g in plan] or
               [int(lib.nm_normative_centile_workspace(0, D))])
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    max_rows = _max_rows(mats)
    if len(plan) <= 1:                                            # one call: the table as it stands, the kernel writes every column row
        for k in range(n_sets):
            full[k].row_off = starts.get(k, 0)
        rf = torch.tensor(ref, dtype=torch.int32, device=dev) if ref_of is not None else None
        sets = _to_dev(full, dev)
        cols = torch.empty(n_sets, D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
        _lib.check(lib.nm_normative_centile(sets.data_ptr(), n_sets, D, max_rows, total, rf.data_ptr() if rf is not None else None,
                                            tail, int(bool(loo)), ws.data_ptr(), need, rows.data_ptr(), cols.data_ptr(),
                                            _stream_ptr(dev)), "nm_normative_centile")
        return zs, rows[:total], cols
    cols = torch.full((n_sets, D, _lib.NM_METRICS_STRIDE), float("nan"), dtype=torch.float64, device=dev)
    for g in plan:
        members = list(g) + sorted({ref[k] for k in g} - set(g))          # the group's scored sets, then references only
        local = {k: i for i, k in enumerate(members)}
        table = (_lib.NmNormSet * len(members))()
        g_rows = 0
        for i, k in enumerate(members):
            C.memmove(C.byref(table, i * C.sizeof(_lib.NmNormSet)), C.byref(full, k * C.sizeof(_lib.NmNormSet)),
                      C.sizeof(_lib.NmNormSet))
            table[i].row_off = g_rows if i < len(g) else 0
            g_rows += heights[k] if i < len(g) else 0
        rf = torch.tensor([local[ref[k]] for k in g] + [-1] * (len(members) - len(g)), dtype=torch.int32, device=dev)
        sets = _to_dev(table, dev)
        cg = torch.empty(len(members), D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
        _lib.check(lib.nm_normative_centile(sets.data_ptr(), len(members), D, max_rows, g_rows, rf.data_ptr(), tail, int(bool(loo)),
                                            ws.data_ptr(), int(ws.numel()), rows[starts[g[0]]:].data_ptr(), cg.data_ptr(),
                                            _stream_ptr(dev)), "nm_normative_centile")
        cols[torch.tensor(g, device=dev)] = cg[:len(g)]
    return zs, rows[:total], cols


def robust_moments(stats: torch.Tensor, scale: float = 1.4826) -> torch.Tensor:
    """A cohort_quantiles `stats` table as a moments table for normative_z (COHORT_MOMENTS_COLUMNS): mean := median, sd :=
    scale x mad (1.4826 makes the MAD of a normal sample estimate its sd), var := sd^2, n_ref, min and max NaN, n_nonfinite,
    status -2 where the statistics' status is -2 or mad == 0.  A torch expression where `stats` lies; no kernel."""
    scale = float(scale)
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"scale must be finite and > 0, got {scale}")
    if not isinstance(stats, torch.Tensor) or stats.dtype != torch.float64 or stats.dim() != 3 or \
            int(stats.shape[2]) != _lib.NM_METRICS_STRIDE:
        raise ValueError(f"stats must be a float64 [n, D, {_lib.NM_METRICS_STRIDE}] tensor as cohort_quantiles returns it")
    med, mad = stats[..., 0], stats[..., 1]
    sd = scale * mad
    nan = torch.full_like(med, float("nan"))
    bad = (stats[..., 7] == -2.0) | (mad == 0.0)
    status = torch.where(bad, torch.full_like(med, -2.0), torch.zeros_like(med))
    return torch.stack([med, sd, sd * sd, stats[..., 5], nan, nan, stats[..., 6], status], dim=-1)


FIT_COLUMNS = ("rho", "p_rho", "smse", "expv", "msll", "rmse", "n_obs", "status")
CALIBRATION_COLUMNS = ("bias", "mae", "mean_z", "sd_z", "skew_z", "kurt_z", "coverage", "n_var")
FIT_RANK_COLUMNS = ("spearman", "p_spearman", "t_spearman", "n_obs", "n_tied_y", "n_tied_loc", "reserved", "status")


def _fit_check(mats, locs, groups, var, col_var, moments, ref_of, thr):
    """nm_fit_quality's argument checks on the host (no device is looked for): D, thr, ref_of as a list or None."""
    thr = float(thr)
    if not (np.isfinite(thr) and thr > 0.0):
        raise ValueError(f"thr must be finite and > 0, got {thr}")
    D = _table_check(mats, groups)
    for name, seq in (("locs", locs), ("var", var)):
        if seq is None:
            if name == "locs":
                raise ValueError("locs is needed: one prediction table per set")
            continue
        if len(seq) != len(mats):
            raise ValueError(f"{name} must have one entry per set")
        for k, (m, b) in enumerate(zip(mats, seq)):
            if b is None and name == "var":                          # (a set without a per-element variance)
                continue
            if not isinstance(b, torch.Tensor) or b.dtype != torch.float32 or b.shape != m.shape:
                raise ValueError(f"set {k}: {name} must be a float32 tensor of the table's shape {tuple(m.shape)}")
            if b.shape[0] > 0 and b.stride(1) != 1:
                raise ValueError(f"set {k}: the columns of {name} must be contiguous")
            if b.shape[0] > 1 and b.stride(0) < D:
                raise ValueError(f"set {k}: row stride {b.stride(0)} of {name} below the {D} columns")
            if b.device != m.device:
                raise ValueError(f"set {k}: {name} is on {b.device}, the table on {m.device}")
    if col_var is not None:
        if len(col_var) != len(mats):
            raise ValueError("col_var must have one entry per set")
        for k, c in enumerate(col_var):
            if c is not None and int(torch.as_tensor(c).numel()) != D:
                raise ValueError(f"set {k}: col_var must hold one variance per column ({D})")
    ref = None
    if moments is None:
        if ref_of is not None:
            raise ValueError("ref_of needs moments")
    else:
        if not isinstance(moments, torch.Tensor) or moments.dtype != torch.float64 or moments.dim() != 3 or \
                int(moments.shape[0]) < 1 or tuple(moments.shape[1:]) != (D, _lib.NM_METRICS_STRIDE):
            raise ValueError(f"moments must be a float64 [n >= 1, {D}, {_lib.NM_METRICS_STRIDE}] tensor as cohort_moments returns it")
        ref = _ref_check(ref_of, len(mats), int(moments.shape[0]), lowest=-1)
    return D, thr, ref


def fit_quality(mats: Sequence[torch.Tensor], locs: Sequence[torch.Tensor], groups: Sequence, var: Optional[Sequence[torch.Tensor]] = None,
                col_var: Optional[Sequence] = None, moments: Optional[torch.Tensor] = None, ref_of=None, thr: float = 1.96,
                rank: bool = False, device=None):
    """(fit, cal), or (fit, cal, rank) with rank=True: each [n_sets, D, 8] fp64 on the device, per (set, column) over the rows
    whose group word is 0 (the hold-out controls) -- does the model predict the column, and is its predictive variance honest?
    fit = rho, p_rho, smse, expv, msll, rmse, n_obs, status (FIT_COLUMNS); cal = bias, mae, mean_z, sd_z, skew_z, kurt_z,
    coverage, n_var (CALIBRATION_COLUMNS); rank = spearman, p_spearman, t_spearman, n_obs, n_tied_y, n_tied_loc, 0, status
    (FIT_RANK_COLUMNS); include/nmhip.h has the definitions.  mats[k]: the observed [n_k, D] fp32 device table, read where it
    lies, as for roi_effect; locs[k]: the prediction, the same shape; var[k] (optional, the same shape, or None for a set): the
    per-element predictive variance; col_var[k] (optional, [D], or None for a set): a per-column variance added to it (exp(logvar_out));
    z = (x - loc) / sqrt(var + col_var).  moments (optional, [n, D, 8] as cohort_moments returns it, formed with ddof=0 on the
    train cohort) is the trivial model of msll, set k against row ref_of[k] (default k; -1: none).  status -2: fewer than two
    evaluated rows, a non-finite value among them, a constant column; else bits 1 (a constant prediction, or n < 3), 2 (no
    usable variance: msll and the z columns NaN), 4 (no trivial model: msll NaN).  One launch for all sets, one more for rank."""
    D, thr, ref = _fit_check(mats, locs, groups, var, col_var, moments, ref_of, thr)
    dev = _table_device(mats, device)
    grp = _row_words(groups, dev, torch.int32)
    cvs = _row_words(col_var, dev, torch.float32) if col_var is not None else None
    sets = _to_dev(_fit_table(mats, locs, grp, var, cvs), dev)
    mom = moments.to(dev).contiguous() if moments is not None else None
    rf = torch.tensor(ref, dtype=torch.int32, device=dev) if ref is not None else None
    n_sets, max_rows, lib = len(mats), _max_rows(mats), _lib.load()
    fit = torch.empty(n_sets, D, _lib.NM_METRICS_STRIDE, dtype=torch.float64, device=dev)
    cal = torch.empty_like(fit)
    _lib.check(lib.nm_fit_quality(sets.data_ptr(), n_sets, D, max_rows, mom.data_ptr() if mom is not None else None,
                                  int(mom.shape[0]) if mom is not None else 0, rf.data_ptr() if rf is not None else None, thr,
                                  fit.data_ptr(), cal.data_ptr(), _stream_ptr(dev)), "nm_fit_quality")
    if not rank:
        return fit, cal
    rk = torch.empty_like(fit)
    _lib.check(lib.nm_fit_rank(sets.data_ptr(), n_sets, D, max_rows, rk.data_ptr(), _stream_ptr(dev)), "nm_fit_rank")
    return fit, cal, rk
