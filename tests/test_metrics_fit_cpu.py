"""metrics.fit_quality refuses malformed input with ValueErrors before it asks for a GPU, its pointer table reads views where
they lie, io.write_fit_csv writes the documented layout, and the sweep's parsers know the new flags.  No GPU here."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from multi_modal_normative_modeling_amd import _lib, io, metrics


def test_value_errors_before_a_gpu_is_asked_for():
    x, g = torch.zeros(6, 5), torch.zeros(6, dtype=torch.int32)
    mom = torch.zeros(2, 5, 8, dtype=torch.float64)
    good = dict(mats=[x], locs=[x], groups=[g])
    bad = [
        dict(mats=[], locs=[], groups=[]), dict(groups=[g, g]), dict(mats=[x.double()]), dict(mats=[x[0]], groups=[g[:1]]),
        dict(mats=[x, torch.zeros(6, 4)], locs=[x, torch.zeros(6, 4)], groups=[g, g]), dict(groups=[g[:5]]),
        dict(mats=[torch.zeros(6, 10)[:, ::2]]),
        dict(mats=[torch.zeros(_lib.NM_METRICS_MAX_N + 1, 5)], locs=[torch.zeros(_lib.NM_METRICS_MAX_N + 1, 5)],
             groups=[torch.zeros(_lib.NM_METRICS_MAX_N + 1)]),
        dict(locs=None), dict(locs=[x, x]), dict(locs=[x.double()]), dict(locs=[torch.zeros(5, 5)]), dict(locs=[np.zeros((6, 5), np.float32)]),
        dict(locs=[torch.zeros(6, 10)[:, ::2]]),
        dict(var=[x, x]), dict(var=[x.double()]), dict(var=[torch.zeros(6, 4)]), dict(var=[torch.zeros(6, 10)[:, ::2]]),
        dict(col_var=[torch.zeros(5), torch.zeros(5)]), dict(col_var=[torch.zeros(4)]),
        dict(thr=0.0), dict(thr=-2.0), dict(thr=float("nan")), dict(thr=float("inf")),
        dict(ref_of=[0]),                                                  # ref_of without moments
        dict(moments=mom.float()), dict(moments=torch.zeros(2, 4, 8, dtype=torch.float64)), dict(moments=mom[0]),
        dict(moments=mom[:0]), dict(moments=mom, ref_of=[0, 0]), dict(moments=mom, ref_of=[2]), dict(moments=mom, ref_of=[-2]),
        dict(mats=[x, x, x], locs=[x, x, x], groups=[g, g, g], moments=mom),  # three sets, two moments rows, no ref_of
    ]
    for b in bad:
        with pytest.raises(ValueError):
            metrics.fit_quality(**{**good, **b})
    if not torch.cuda.is_available():                                 # well-formed input, no GPU: no quiet host path
        for kw in (dict(), dict(var=[x], col_var=[torch.ones(5)], moments=mom, ref_of=[-1], rank=True)):
            with pytest.raises(_lib.NmError):
                metrics.fit_quality(**{**good, **kw})


def test_pointer_table_reads_views_where_they_lie():
    buf, loc, var = torch.zeros(40, 12), torch.zeros(40, 16), torch.zeros(40, 9)
    g, cv = torch.zeros(40, dtype=torch.int32), torch.ones(9)
    views = [buf[:, :9], buf[5:31, :9], buf[7:8, :9], buf[:0, :9]]
    locs = [loc[:, :9], loc[5:31, :9], loc[7:8, :9], loc[:0, :9]]
    vars_ = [var, var[5:31], None, var[:0]]
    table = metrics._fit_table(views, locs, [g[:len(v)] for v in views], vars_, [cv, None, cv, cv])
    assert C.sizeof(table) == 4 * 56
    assert [t.x for t in table] == [buf.data_ptr(), buf.data_ptr() + 5 * 12 * 4, buf.data_ptr() + 7 * 12 * 4, None]
    assert [t.loc for t in table] == [loc.data_ptr(), loc.data_ptr() + 5 * 16 * 4, loc.data_ptr() + 7 * 16 * 4, None]
    assert [t.var for t in table] == [var.data_ptr(), var.data_ptr() + 5 * 9 * 4, None, None]
    assert [t.col_var for t in table] == [cv.data_ptr(), None, cv.data_ptr(), None]
    assert [t.rows for t in table] == [40, 26, 1, 0]
    assert [t.pitch for t in table] == [12, 12, 9, 9] and [t.loc_pitch for t in table] == [16, 16, 9, 0]
    assert [t.var_pitch for t in table] == [9, 9, 0, 0] and table[0].group == g.data_ptr() and table[3].group is None
    bare = metrics._fit_table(views, locs, [g[:len(v)] for v in views])
    assert all(t.var is None and t.col_var is None and t.var_pitch == 0 for t in bare)


def test_write_fit_csv_layout(tmp_path):
    rng = np.random.default_rng(0)
    fit, cal, rank = rng.normal(size=(3, 8)), rng.normal(size=(3, 8)), rng.normal(size=(3, 8))
    fit[1, 4] = np.nan
    rois = ["a", "b", "c"]
    path = io.write_fit_csv(tmp_path / "m", "T1w", rois, fit, cal)
    assert path == tmp_path / "m" / "fit_quality_T1w.csv"
    df = pd.read_csv(path, float_precision="round_trip")
    assert list(df.columns) == ["ROI"] + list(metrics.FIT_COLUMNS) + list(metrics.CALIBRATION_COLUMNS)
    assert list(df["ROI"]) == rois
    got = df.iloc[:, 1:].to_numpy(dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(np.c_[fit, cal])) and np.allclose(got, np.c_[fit, cal], rtol=0, atol=0, equal_nan=True)
    df = pd.read_csv(io.write_fit_csv(tmp_path / "m", "T1w", rois, fit, cal, rank), float_precision="round_trip")
    assert list(df.columns) == ["ROI"] + io.fit_csv_columns(rank=True) and len(set(df.columns)) == 25
    assert list(df.columns[17:]) == ["spearman", "p_spearman", "t_spearman", "n_obs_rank", "n_tied_y", "n_tied_loc", "reserved",
                                     "status_rank"]
    assert np.array_equal(df.iloc[:, 17:].to_numpy(dtype=np.float64), rank)
    for bad in (dict(fit=fit[:2]), dict(cal=cal[:, :7]), dict(rank=rank[:2])):
        with pytest.raises(ValueError):
            io.write_fit_csv(tmp_path / "m", "T1w", rois, **{**dict(fit=fit, cal=cal), **bad})


def test_sweep_parsers_know_the_new_flags(capsys):
    from multi_modal_normative_modeling_amd import sweep
    with pytest.raises(SystemExit) as e:
        sweep.main_test(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--fit " in text.replace("\n", " ") + " " and "--fit-rank" in text
    with pytest.raises(SystemExit) as e:
        sweep.main_analysis(["--help"])
    assert e.value.code == 0 and "--fit" in capsys.readouterr().out
    for argv, why in ((["--fit"], "--fit needs --roi-effect"), (["--roi-effect", "--fit-rank"], "--fit-rank needs --fit")):
        with pytest.raises(SystemExit) as e:
            sweep.main_test(["--models-dir", "nowhere"] + argv)
        assert e.value.code == 2 and why in capsys.readouterr().err, argv
    with pytest.raises(ValueError):
        sweep.test_folds([], None, [], ["a"], "poe", "cpu", fit=True)
    with pytest.raises(ValueError):
        sweep.test_folds([], None, [], ["a"], "poe", "cpu", roi_effect=True, fit_rank=True)
    assert [st.key for st in sweep.ROI_STATS][-1] == "fit"
