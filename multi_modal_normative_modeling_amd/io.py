"""On-disk formats of the deviation pass (same pandas calls as the reference, so the text is
byte-compatible with its tooling).

``deviation_fold_{fold}_{dataset_name}_roiwise.csv``: header ``IID,ROI_0..ROI_{D-1}``, one row per
subject in table order, float32 values  (multimodal_kfold_train_cvae_supervised_regression.py:190-192).
The five CSV kinds of the test script (multimodal_kfold_test_cvae_supervised.py:116-154).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import pandas as pd

from . import prep

META_COLS = ["participant_id", "DIA", "AGE", "PTGENDER"]


def roiwise_filename(fold: int, dataset_name: str) -> str:
    return f"deviation_fold_{fold}_{dataset_name}_roiwise.csv"


def write_roiwise_csv(out_dir, fold: int, dataset_name: str, iids: Sequence[int], deviation_roi: np.ndarray) -> Path:
    dev = np.asarray(deviation_roi, dtype=np.float32)
    df_out = pd.DataFrame(dev, columns=[f"ROI_{i}" for i in range(dev.shape[1])])
    df_out.insert(0, "IID", list(iids))
    path = Path(out_dir) / roiwise_filename(fold, dataset_name)
    path.parent.mkdir(parents=True, exist_ok=True)
    df_out.to_csv(path, index=False)
    return path


def write_test_csvs(out_dir, dataset_name: str, covariates: pd.DataFrame, roi_columns: Sequence[str], x: np.ndarray,
                    x_hat: np.ndarray) -> Dict[str, Path]:
    """normalized_ / reconstruction_ / reconstruction_error_ / reconstruction_error_roi_ /
    deviation_as_feature_importance_{name}.csv with the reference's column layouts."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    cov = covariates[META_COLS].copy()
    paths = {}
    cov = cov.reset_index(drop=True)

    def with_rois(values):                      # same frame as `df[columns_name] = values` (…test….py:123-124), built in one go
        return pd.concat([cov, pd.DataFrame(np.asarray(values), columns=list(roi_columns))], axis=1)

    normalized = with_rois(x)
    paths["normalized"] = out_dir / f"normalized_{dataset_name}.csv"
    normalized.to_csv(paths["normalized"], index=False)
    recon = with_rois(x_hat)
    paths["reconstruction"] = out_dir / f"reconstruction_{dataset_name}.csv"
    recon.to_csv(paths["reconstruction"], index=False)
    err = cov.copy()
    err["Reconstruction error"] = np.sum((x - x_hat) ** 2, axis=1) / x.shape[1]
    paths["reconstruction_error"] = out_dir / f"reconstruction_error_{dataset_name}.csv"
    err.to_csv(paths["reconstruction_error"], index=False)
    err_roi = with_rois((x - x_hat) ** 2)
    paths["reconstruction_error_roi"] = out_dir / f"reconstruction_error_roi_{dataset_name}.csv"
    err_roi.to_csv(paths["reconstruction_error_roi"], index=False)
    fi = err_roi.rename(columns=dict(zip(roi_columns, map(str, range(1, len(roi_columns) + 1)))))
    paths["deviation_as_feature_importance"] = out_dir / f"deviation_as_feature_importance_{dataset_name}.csv"
    fi.to_csv(paths["deviation_as_feature_importance"], index=False)
    return paths


def given_filename(dataset_name: str, tag: str) -> str:
    """The per-subject error of modality `dataset_name` reconstructed from the modalities of `tag` (their names joined by +)."""
    return f"reconstruction_error_{dataset_name}_given_{tag}.csv"


def write_given_csv(out_dir, dataset_name: str, tag: str, covariates: pd.DataFrame, x: np.ndarray, x_hat: np.ndarray) -> Path:
    """reconstruction_error_<name>_given_<tag>.csv in the layout of reconstruction_error_<name>.csv (write_test_csvs): the
    metadata columns and `Reconstruction error`, the row mean of (x - x_hat)^2 formed the same way -- x_hat here the
    reconstruction from the joint latent of the modalities in `tag` alone (sweep.test_folds(given=...))."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    err = covariates[META_COLS].copy().reset_index(drop=True)
    err["Reconstruction error"] = np.sum((x - x_hat) ** 2, axis=1) / x.shape[1]
    path = out_dir / given_filename(dataset_name, tag)
    err.to_csv(path, index=False)
    return path


PREDICTIVE_KINDS = ("reconstruction_mc", "reconstruction_error_roi_mc", "reconstruction_error_mc", "predictive_z", "predictive_subject")


def write_predictive_csvs(out_dir, dataset_name: str, covariates: pd.DataFrame, roi_columns: Sequence[str], mean: np.ndarray,
                          msq: np.ndarray, z: np.ndarray) -> Dict[str, Path]:
    """The files of the posterior-predictive pass (sweep.test_folds(draws=S)), next to the five kinds of write_test_csvs and in
    their layouts: reconstruction_mc_ (the mean reconstruction over the draws), reconstruction_error_roi_mc_ (per ROI the
    Monte-Carlo mean of (x - x_hat_s)^2), reconstruction_error_mc_ (its row mean, formed as reconstruction_error_ forms its
    own: one draw gives that file byte for byte), predictive_z_ (per ROI (x - mean) / sqrt(exp(logvar_out) + the draw
    variance)) and predictive_subject_ (per subject the mean squared error, the mean z^2, the largest |z| and its ROI)."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    cov = covariates[META_COLS].copy().reset_index(drop=True)
    frames = {}
    for kind, values in (("reconstruction_mc", mean), ("reconstruction_error_roi_mc", msq), ("predictive_z", z)):
        frames[kind] = pd.concat([cov, pd.DataFrame(np.asarray(values), columns=list(roi_columns))], axis=1)
    err = cov.copy()
    err["Reconstruction error"] = np.sum(msq, axis=1) / msq.shape[1]
    frames["reconstruction_error_mc"] = err
    sub = cov.copy()
    worst = np.argmax(np.abs(z), axis=1)
    sub["Mean squared error"] = err["Reconstruction error"]
    sub["Mean z2"] = np.sum(z * z, axis=1) / z.shape[1]
    sub["Max abs z"] = np.abs(z)[np.arange(len(z)), worst]
    sub["Max abs z ROI"] = [roi_columns[i] for i in worst]
    frames["predictive_subject"] = sub
    paths = {}
    for kind in PREDICTIVE_KINDS:
        paths[kind] = out_dir / f"{kind}_{dataset_name}.csv"
        frames[kind].to_csv(paths[kind], index=False)
    return paths


def write_loglik_csv(out_dir, name: str, covariates: pd.DataFrame, row: np.ndarray, columns: Sequence[str],
                     recon_ll: Dict[str, np.ndarray]) -> Path:
    """loglik_<name>.csv of the likelihood pass (sweep.test_folds(loglik=S)): the metadata columns of write_test_csvs, the
    columns of the pass's row export (metrics.LOGLIK_ROW_COLUMNS: log_px, elbo, ess, kl_mc, kl, recon_ll, logw_max, logw_min)
    and recon_ll_<m> per modality -- one file per procedure, the model's own log p(x | c) of every test subject."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    df = covariates[META_COLS].copy().reset_index(drop=True)
    for j, c in enumerate(columns):
        df[c] = np.asarray(row)[:, j]
    for m, v in recon_ll.items():
        df[f"recon_ll_{m}"] = np.asarray(v)
    path = out_dir / f"loglik_{name}.csv"
    df.to_csv(path, index=False)
    return path


def write_latent_csvs(out_dir, name: str, covariates: pd.DataFrame, mu: np.ndarray, var: np.ndarray, score: np.ndarray,
                      zsep: np.ndarray) -> Dict[str, Path]:
    """The latent-space deviation of one fold's test subjects (pred_latent + latent_deviation / separate_latent_deviation,
    utils_vae.py:155-161), with the metadata columns of write_test_csvs:
      latent_{name}.csv            participant_id, DIA, AGE, PTGENDER, mu_0.., var_0..   (the joint posterior)
      latent_deviation_{name}.csv  participant_id, DIA, AGE, PTGENDER, Latent deviation, z_0..z_{Z-1}"""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    cov = covariates[META_COLS].copy().reset_index(drop=True)
    Z = int(np.asarray(mu).shape[1])
    paths = {"latent": out_dir / f"latent_{name}.csv", "latent_deviation": out_dir / f"latent_deviation_{name}.csv"}
    pd.concat([cov, pd.DataFrame(np.asarray(mu), columns=[f"mu_{i}" for i in range(Z)]),
               pd.DataFrame(np.asarray(var), columns=[f"var_{i}" for i in range(Z)])], axis=1).to_csv(paths["latent"], index=False)
    dev = cov.copy()
    dev["Latent deviation"] = np.asarray(score)
    pd.concat([dev, pd.DataFrame(np.asarray(zsep), columns=[f"z_{i}" for i in range(Z)])], axis=1).to_csv(
        paths["latent_deviation"], index=False)
    return paths


def write_roi_table_csv(kind: str, out_dir, dataset_name: str, roi_columns: Sequence[str], table: np.ndarray,
                        columns: Optional[Sequence[str]] = None) -> Path:
    """{kind}_{name}.csv, kind one of roi_effect / roi_significance / roi_regress / centile_map: one row per ROI -- its column
    name, then the kind's eight metrics columns (ROI_EFFECT_COLUMNS / ROI_SIGNIFICANCE_COLUMNS / COLUMN_REGRESS_COLUMNS /
    CENTILE_COL_COLUMNS); any other kind names its `columns` itself (centile_curve: the quantiles it was asked for)."""
    from . import metrics
    if columns is None:
        columns = {"roi_effect": metrics.ROI_EFFECT_COLUMNS, "roi_significance": metrics.ROI_SIGNIFICANCE_COLUMNS,
                   "roi_regress": metrics.COLUMN_REGRESS_COLUMNS, "centile_map": metrics.CENTILE_COL_COLUMNS}[kind]
    table = np.asarray(table, dtype=np.float64)
    if table.shape != (len(roi_columns), len(columns)):
        raise ValueError(f"a [{len(roi_columns)}, {len(columns)}] table is needed, got {table.shape}")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    df = pd.DataFrame(table, columns=list(columns))
    df.insert(0, "ROI", list(roi_columns))
    path = out_dir / f"{kind}_{dataset_name}.csv"
    df.to_csv(path, index=False)
    return path


def write_roi_effect_csv(out_dir, dataset_name: str, roi_columns: Sequence[str], table: np.ndarray) -> Path:
    """roi_effect_{name}.csv: one row per ROI -- its column name, then metrics.ROI_EFFECT_COLUMNS (Cliff's delta of patients
    against controls on the ROI's squared error, its ROC-AUC, the pair counts, group sizes and group means)."""
    return write_roi_table_csv("roi_effect", out_dir, dataset_name, roi_columns, table)


def write_roi_significance_csv(out_dir, dataset_name: str, roi_columns: Sequence[str], table: np.ndarray) -> Path:
    """roi_significance_{name}.csv: one row per ROI -- its column name, then metrics.ROI_SIGNIFICANCE_COLUMNS (the
    Mann-Whitney U of patients against controls on the ROI's squared error, its tie term, z and asymptotic p, the
    Benjamini-Hochberg q over the ROIs, the label-permutation p of the ROI and against the maximum over the ROIs, and the
    number of permutations).  The subjects are taken as independent."""
    return write_roi_table_csv("roi_significance", out_dir, dataset_name, roi_columns, table)


def write_roi_regress_csv(out_dir, dataset_name: str, roi_columns: Sequence[str], table: np.ndarray) -> Path:
    """roi_regress_{name}.csv: one row per ROI -- its column name, then metrics.COLUMN_REGRESS_COLUMNS (the fit
    target ~ const + the ROI's squared error + the adjustment covariates: both reported parameters, their standard errors
    and p-values, the subjects that took part and the Newton steps; n_iter < 0 is a status, see metrics.column_regress)."""
    return write_roi_table_csv("roi_regress", out_dir, dataset_name, roi_columns, table)


def fit_csv_columns(rank: bool = False) -> list:
    """The columns of fit_quality_{name}.csv after "ROI": metrics.FIT_COLUMNS, metrics.CALIBRATION_COLUMNS and, with rank,
    metrics.FIT_RANK_COLUMNS -- a name the rank table shares with the fit table (n_obs, status) carries the suffix _rank."""
    from . import metrics
    cols = list(metrics.FIT_COLUMNS) + list(metrics.CALIBRATION_COLUMNS)
    if rank:
        cols += [c + "_rank" if c in cols else c for c in metrics.FIT_RANK_COLUMNS]
    return cols


def write_fit_csv(out_dir, dataset_name: str, roi_columns: Sequence[str], fit: np.ndarray, cal: np.ndarray,
                  rank: Optional[np.ndarray] = None) -> Path:
    """fit_quality_{name}.csv: one row per ROI -- its column name, then fit_csv_columns(): the model's fit on the hold-out
    controls (rho, p_rho, smse, expv, msll, rmse, n_obs, status), the calibration of its z (bias, mae, mean_z, sd_z, skew_z,
    kurt_z, coverage, n_var) and, where the rank table was asked for, Spearman's rho with its p, t, n and tie counts."""
    tabs = [np.asarray(v, dtype=np.float64) for v in (fit, cal) + (() if rank is None else (rank,))]
    for v in tabs:
        if v.shape != (len(roi_columns), 8):
            raise ValueError(f"[{len(roi_columns)}, 8] tables are needed, got {v.shape}")
    return write_roi_table_csv("fit_quality", out_dir, dataset_name, roi_columns, np.concatenate(tabs, axis=1),
                               columns=fit_csv_columns(rank is not None))


def write_normative_csvs(out_dir, dataset_name: str, covariates: pd.DataFrame, roi_columns: Sequence[str], z: np.ndarray,
                         rows: np.ndarray, cols: np.ndarray) -> Dict[str, Path]:
    """The normative z-map of one set of subjects (metrics.normative_z), with the metadata columns of write_test_csvs:
      normative_z_{name}.csv        participant_id, DIA, AGE, PTGENDER, then one z per ROI
      normative_subject_{name}.csv  participant_id, DIA, AGE, PTGENDER, then metrics.NORMATIVE_ROW_COLUMNS
      normative_map_{name}.csv      ROI, then metrics.NORMATIVE_COL_COLUMNS (the extreme-deviation map)"""
    return _write_z_map_csvs("normative", out_dir, dataset_name, covariates, roi_columns, z, rows, cols)


def _write_z_map_csvs(prefix: str, out_dir, dataset_name: str, covariates: pd.DataFrame, roi_columns: Sequence[str], z, rows, cols):
    """{prefix}_z / _subject / _map _{name}.csv: the three files of a z-map (write_normative_csvs, write_trajectory_csvs)."""
    from .metrics import NORMATIVE_COL_COLUMNS, NORMATIVE_ROW_COLUMNS
    z, rows, cols = np.asarray(z), np.asarray(rows, dtype=np.float64), np.asarray(cols, dtype=np.float64)
    if z.shape != (len(covariates), len(roi_columns)) or rows.shape != (len(covariates), len(NORMATIVE_ROW_COLUMNS)) or \
            cols.shape != (len(roi_columns), len(NORMATIVE_COL_COLUMNS)):
        raise ValueError(f"z [{len(covariates)}, {len(roi_columns)}], rows [{len(covariates)}, 8] and cols [{len(roi_columns)}, 8] "
                         f"are needed, got {z.shape}, {rows.shape}, {cols.shape}")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    cov = covariates[META_COLS].copy().reset_index(drop=True)
    paths = {k: out_dir / f"{prefix}_{k}_{dataset_name}.csv" for k in ("z", "subject", "map")}
    pd.concat([cov, pd.DataFrame(z, columns=list(roi_columns))], axis=1).to_csv(paths["z"], index=False)
    pd.concat([cov, pd.DataFrame(rows, columns=list(NORMATIVE_ROW_COLUMNS))], axis=1).to_csv(paths["subject"], index=False)
    df = pd.DataFrame(cols, columns=list(NORMATIVE_COL_COLUMNS))
    df.insert(0, "ROI", list(roi_columns))
    df.to_csv(paths["map"], index=False)
    return paths


TRAJECTORY_CHART_COLUMNS = ["cell", "age_bin", "gender_bin", "age_lo", "age_hi", "n_test"]


def write_trajectory_chart_csvs(out_dir, dataset_name: str, roi_columns: Sequence[str], cells: pd.DataFrame, mean: np.ndarray,
                                sd: np.ndarray) -> Dict[str, Path]:
    """The normative chart of one fold and modality (the model's expectation per covariate cell), one row per cell:
      normative_trajectory_mean_{name}.csv  cell, age_bin, gender_bin, age_lo, age_hi, n_test, then the mean per ROI
      normative_trajectory_sd_{name}.csv    the same columns, then the predictive sd per ROI
    cells: a frame with TRAJECTORY_CHART_COLUMNS (age_lo / age_hi NaN -- an empty field -- where no test subject is in the bin)."""
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    if list(cells.columns) != TRAJECTORY_CHART_COLUMNS or mean.shape != (len(cells), len(roi_columns)) or sd.shape != mean.shape:
        raise ValueError(f"cells with {TRAJECTORY_CHART_COLUMNS} and mean / sd [{len(cells)}, {len(roi_columns)}] are needed, got "
                         f"{list(cells.columns)}, {mean.shape}, {sd.shape}")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    head = cells.reset_index(drop=True)
    paths = {k: out_dir / f"normative_trajectory_{k}_{dataset_name}.csv" for k in ("mean", "sd")}
    for k, tab in (("mean", mean), ("sd", sd)):
        pd.concat([head, pd.DataFrame(tab, columns=list(roi_columns))], axis=1).to_csv(paths[k], index=False)
    return paths


def write_trajectory_csvs(out_dir, dataset_name: str, covariates: pd.DataFrame, roi_columns: Sequence[str], z: np.ndarray,
                          rows: np.ndarray, cols: np.ndarray) -> Dict[str, Path]:
    """The trajectory z-scores of one set of subjects -- every ROI against the chart row of the subject's own cell -- in the
    layouts of write_normative_csvs: trajectory_z_{name}.csv, trajectory_subject_{name}.csv (metrics.NORMATIVE_ROW_COLUMNS)
    and trajectory_map_{name}.csv (metrics.NORMATIVE_COL_COLUMNS, summed over the cells)."""
    return _write_z_map_csvs("trajectory", out_dir, dataset_name, covariates, roi_columns, z, rows, cols)


def quantile_column(p: float) -> str:
    """The column name of the quantile at probability p in centile_curve_{name}.csv: q_0.05, q_0.5, ..."""
    return f"q_{float(p):g}"


def write_centile_csvs(out_dir, dataset_name: str, covariates: pd.DataFrame, roi_columns: Sequence[str], pct: np.ndarray,
                       rows: np.ndarray, cols: np.ndarray, probs: Sequence[float], q: np.ndarray, stats: np.ndarray) -> Dict[str, Path]:
    """The normative centiles of one set of subjects (metrics.normative_centile / cohort_quantiles), with the metadata
    columns of write_test_csvs; the two per-ROI files go through write_roi_table_csv:
      centile_pct_{name}.csv      participant_id, DIA, AGE, PTGENDER, then one percentile rank per ROI
      centile_subject_{name}.csv  participant_id, DIA, AGE, PTGENDER, then metrics.CENTILE_ROW_COLUMNS
      centile_map_{name}.csv      ROI, then metrics.CENTILE_COL_COLUMNS (the extreme-centile map)
      centile_curve_{name}.csv    ROI, then the quantiles asked for (q_<p>) and metrics.COHORT_QUANTILE_COLUMNS of the
                                  reference cohort: the normative range"""
    from .metrics import CENTILE_ROW_COLUMNS, COHORT_QUANTILE_COLUMNS
    pct, rows = np.asarray(pct), np.asarray(rows, dtype=np.float64)
    q, stats = np.asarray(q, dtype=np.float64), np.asarray(stats, dtype=np.float64)
    probs = [float(p) for p in probs]
    n, D = len(covariates), len(roi_columns)
    if pct.shape != (n, D) or rows.shape != (n, len(CENTILE_ROW_COLUMNS)) or q.shape != (D, len(probs)) or \
            stats.shape != (D, len(COHORT_QUANTILE_COLUMNS)):
        raise ValueError(f"pct [{n}, {D}], rows [{n}, 8], q [{D}, {len(probs)}] and stats [{D}, 8] are needed, got {pct.shape}, "
                         f"{rows.shape}, {q.shape}, {stats.shape}")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    cov = covariates[META_COLS].copy().reset_index(drop=True)
    paths = {k: out_dir / f"centile_{k}_{dataset_name}.csv" for k in ("pct", "subject")}
    pd.concat([cov, pd.DataFrame(pct, columns=list(roi_columns))], axis=1).to_csv(paths["pct"], index=False)
    pd.concat([cov, pd.DataFrame(rows, columns=list(CENTILE_ROW_COLUMNS))], axis=1).to_csv(paths["subject"], index=False)
    paths["map"] = write_roi_table_csv("centile_map", out_dir, dataset_name, roi_columns, cols)
    paths["curve"] = write_roi_table_csv("centile_curve", out_dir, dataset_name, roi_columns, np.concatenate([q, stats], axis=1),
                                         columns=[quantile_column(p) for p in probs] + list(COHORT_QUANTILE_COLUMNS))
    return paths


def write_latent_mahalanobis_csv(out_dir, name: str, covariates: pd.DataFrame, d: np.ndarray) -> Path:
    """latent_mahalanobis_{name}.csv: participant_id, DIA, AGE, PTGENDER, d2, d -- the Mahalanobis distance of every test
    subject's joint mu to the fold's train cohort (metrics.cohort_cov / metrics.mahalanobis), next to latent_deviation_{name}.csv."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    df = covariates[META_COLS].copy().reset_index(drop=True)
    d = np.asarray(d, dtype=np.float64)
    df["d2"] = d * d
    df["d"] = d
    path = out_dir / f"latent_mahalanobis_{name}.csv"
    df.to_csv(path, index=False)
    return path


def latent_pvalues_frame(table: np.ndarray) -> pd.DataFrame:
    """The DataFrame latent_pvalues returns (utils_vae.py:163-174) from a [Z, 8] metrics.column_regress table: labels =
    ['const', 'latent'], one column 'latent i' per latent dimension with the two p-values."""
    table = np.asarray(table, dtype=np.float64)
    df = pd.DataFrame({"labels": ["const", "latent"]})
    for i in range(table.shape[0]):
        df["latent {0}".format(i)] = [float(table[i, 4]), float(table[i, 5])]
    return df


def write_latent_pvalues_csv(out_dir, name: str, target: str, table: np.ndarray) -> Path:
    """latent_pvalues_{name}_{target}.csv: latent_pvalues_frame of the table, as the reference's frame goes to a file."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    path = out_dir / f"latent_pvalues_{name}_{target}.csv"
    latent_pvalues_frame(table).to_csv(path, index=False)
    return path


# ---- the reference's input layout -----------------------------------------------------------
# data/<resource>/y.csv: IID, participant_id, DIA, AGE, PTGENDER (+ FI for HCPimage); data/<resource>/<modality>.csv:
# IID + the ROI columns.  multimodal_kfold_train_cvae_supervised.py:49-50, 84-91 and utils.py:110-168 read them per
# fold and modality through pd.merge on IID; here they are read once into a prep.Cohort.
_NON_ROI = ("IID", "participant_id", "DIA", "AGE", "PTGENDER", "FI", "Session_ID", "Run_ID")


def read_cohort(resource_dir, resource: str = "HCPimage", modalities: Optional[Sequence[str]] = None) -> prep.Cohort:
    """y.csv (rows with missing values dropped, utils.py:124) inner-merged on IID with every modality table of the
    resource (get_datasets_name order).  Rows follow the first modality's file (pd.merge keeps the left table's order,
    utils.py:117); the other modalities are aligned to it by IID -- the reference feeds the modalities' DataLoaders side by
    side and so assumes the files agree.  ROI columns = every column of the modality file that is not an id / covariate,
    in file order.  DIA is mapped to the cohort's convention 1 = healthy control through get_hc_label (utils.py:760-774).
    A missing FI column (only HCPimage carries it) reads as zeros."""
    resource_dir = Path(resource_dir)
    if resource not in prep.DATASET_MODALITIES:
        raise ValueError("Unknown dataset: {}".format(resource))
    names = list(modalities) if modalities is not None else [m for m in prep.DATASET_MODALITIES[resource]
                                                             if (resource_dir / f"{m}.csv").exists()]
    if not names:
        raise FileNotFoundError(f"no modality tables of {resource} under {resource_dir}")
    y = pd.read_csv(resource_dir / "y.csv").dropna()
    for col in ("IID", "DIA", "AGE", "PTGENDER"):
        if col not in y.columns:
            raise ValueError(f"{resource_dir / 'y.csv'} has no column {col!r}")
    tables = {m: pd.read_csv(resource_dir / f"{m}.csv") for m in names}
    keep = set(y["IID"])
    for t in tables.values():
        keep &= set(t["IID"])
    first = tables[names[0]]
    order = [i for i in first["IID"].tolist() if i in keep]
    if len(set(order)) != len(order):
        raise ValueError(f"{names[0]}.csv repeats IIDs")
    yi = y.drop_duplicates("IID").set_index("IID").loc[order]
    x = {}
    for m, t in tables.items():
        roi = [c for c in t.columns if c not in _NON_ROI]
        x[m] = t.drop_duplicates("IID").set_index("IID").loc[order, roi].to_numpy(dtype=np.float64)
    hc = prep.HC_LABEL[resource]
    fi = yi["FI"].to_numpy(dtype=np.float64) if "FI" in yi.columns else np.zeros(len(order))
    return prep.Cohort(iid=np.asarray(order), age=yi["AGE"].to_numpy(dtype=np.float64), gender=yi["PTGENDER"].to_numpy(dtype=np.float64),
                       dia=(yi["DIA"].to_numpy() == hc).astype(np.int64), fi=fi, x=x, resource=resource)


def write_cohort(cohort: prep.Cohort, resource_dir, roi_names: Optional[dict] = None) -> None:
    """The inverse of read_cohort: a cohort (e.g. the synthetic one) in the reference's ./data/<resource>/ layout, plus
    the early-fusion table the way early_fusion_modalities.py:23-35 builds it (columns `<roi>_<modality>`, modality-major)."""
    resource_dir = Path(resource_dir)
    resource_dir.mkdir(parents=True, exist_ok=True)
    hc = prep.HC_LABEL[cohort.resource]
    dia = np.where(np.asarray(cohort.dia) == 1, hc, 0)
    pd.DataFrame({"IID": cohort.iid, "participant_id": cohort.iid, "DIA": dia, "AGE": cohort.age, "PTGENDER": cohort.gender,
                  "FI": cohort.fi}).to_csv(resource_dir / "y.csv", index=False)
    fused = []
    for m, xm in cohort.x.items():
        cols = list(roi_names[m]) if roi_names and m in roi_names else [f"ROI_{i}" for i in range(xm.shape[1])]
        df = pd.DataFrame(xm, columns=cols)
        df.insert(0, "IID", cohort.iid)
        df.to_csv(resource_dir / f"{m}.csv", index=False)
        fused.append(pd.DataFrame(xm, columns=[f"{c}_{m}" for c in cols]))
    fdf = pd.concat(fused, axis=1)
    fdf.insert(0, "IID", cohort.iid)
    fdf.to_csv(resource_dir / f"{cohort.fusion_name}.csv", index=False)
