"""The yardstick of nm_column_regress (tests/column_regress_ref.py) against independent implementations, and the host
compilation of the Student-t tail the kernel calls.  No GPU.

The closeness rule of the GPU tests is 1e-9 (an estimate against max(|ref|, se), se and p relative).  It is derived here: the
yardstick against its own twin with the rows reversed differs by summation order alone, and that distance is held under
1e-11 on every shape; a dropped row moves a result by about 1 / n >= 1e-4."""
import numpy as np
import pytest
from scipy import stats

from multi_modal_normative_modeling_amd import _lib
from tests import column_regress_ref as R


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("n", [3, 7, 64, 1064])
def test_ols_is_linregress(n):
    rng = np.random.default_rng(n)
    x, y, _ = R.make_case(rng, n, 5, 0, "ols")
    tab = R.table(x, y, kind="ols")
    for c in range(5):
        lr = stats.linregress(x[:, c].astype(np.float64), y.astype(np.float64))
        const, coef, se0, se1, _, p1, n_obs, n_iter = tab[c]
        assert abs(coef - lr.slope) <= 1e-9 * max(abs(lr.slope), lr.stderr)
        assert abs(const - lr.intercept) <= 1e-9 * max(abs(lr.intercept), lr.intercept_stderr)
        assert _rel(se1, lr.stderr) <= 1e-9 and _rel(se0, lr.intercept_stderr) <= 1e-9
        assert _rel(p1, lr.pvalue) <= 1e-9
        assert n_obs == n and n_iter == 0


@pytest.mark.parametrize("q", [0, 2])
def test_logit_is_the_maximum_likelihood_fit(q):
    lm = pytest.importorskip("sklearn.linear_model")
    rng = np.random.default_rng(11 + q)
    x, y, cov = R.make_case(rng, 400, 4, q, "logit")
    tab = R.table(x, y, cov, None, "logit")
    assert np.all(tab[:, 7] >= 1)
    for c in range(4):
        Z = np.column_stack([x[:, c]] + ([cov] if q else [])).astype(np.float64)
        fit = lm.LogisticRegression(penalty=None, tol=1e-12, max_iter=10000).fit(Z, y.astype(np.int64))
        print(c, tab[c, :2], fit.intercept_[0], fit.coef_[0, 0])
        assert abs(tab[c, 1] - fit.coef_[0, 0]) <= 1e-5 * max(abs(fit.coef_[0, 0]), tab[c, 3])
        assert abs(tab[c, 0] - fit.intercept_[0]) <= 1e-5 * max(abs(fit.intercept_[0]), tab[c, 2])


@pytest.mark.parametrize("kind", ["ols", "logit"])
def test_twin_with_reversed_rows_is_far_inside_the_bound(kind):
    rng = np.random.default_rng(5)
    worst = 0.0
    for rows in (7, 63, 257, 1064):
        for q in (0, 1, 4):
            x, y, cov = R.make_case(rng, rows, 9, q, kind)
            inc = (rng.random(rows) < 0.9).astype(np.int32) if rows > 60 else None
            a = R.table(x, y, cov, inc, kind)
            b = R.table(x[::-1], y[::-1], None if cov is None else cov[::-1], None if inc is None else inc[::-1], kind)
            worst = max(worst, R.close(a, b, tol=1e-11))
    print("worst twin distance in units of 1e-11:", worst)
    assert worst <= 1.0


def _offset_column():
    """A column offset by 1e4 as fp32 holds it, and the same values with the offset taken off exactly in fp64."""
    rng = np.random.default_rng(21)
    n = 500
    x_off = (rng.normal(size=n) + 1e4).astype(np.float32)
    x_true = x_off.astype(np.float64) - 1e4
    y = (0.7 * x_true + rng.normal(size=n)).astype(np.float32)
    return x_off, x_true, y


def test_raw_normal_equations_miss_the_bound_on_an_offset_column_and_the_centred_form_holds_it():
    x_off, x_true, y = _offset_column()
    truth = R.table(x_true[:, None], y, kind="ols")[0]          # (fp64 values, well conditioned)
    centred = R.table(x_off[:, None], y, kind="ols")[0]
    raw = R.ols_raw(x_off, y)
    err_c = abs(centred[1] - truth[1]) / max(abs(truth[1]), truth[3])
    err_r = abs(raw[1] - truth[1]) / max(abs(truth[1]), truth[3])
    print("slope error: centred", err_c, "raw", err_r)
    assert err_c <= 1e-9 and _rel(centred[3], truth[3]) <= 1e-9 and _rel(centred[5], truth[5]) <= 1e-9
    assert err_r > 1e-9
    # the intercept moves by the offset times the slope
    assert abs(centred[0] - (truth[0] - 1e4 * truth[1])) <= 1e-9 * max(abs(centred[0]), centred[2])


def test_a_perfectly_separated_column_does_not_converge():
    rng = np.random.default_rng(8)
    n = 80
    y = (np.arange(n) % 2).astype(np.float32)
    x = rng.normal(size=(n, 3)).astype(np.float32)
    x[:, 1] = np.where(y == 1, 1.0 + rng.random(n), -1.0 - rng.random(n))
    tab = R.table(x, y, kind="logit")
    assert tab[1, 7] == -1 and np.all(np.isnan(tab[1, :6])) and tab[1, 6] == n
    assert np.all(tab[[0, 2], 7] >= 1) and np.all(np.isfinite(tab[[0, 2], :6]))


def test_invalid_inputs_of_the_yardstick():
    rng = np.random.default_rng(9)
    x, y, cov = R.make_case(rng, 40, 4, 1, "logit")
    x[:, 2] = 3.0                                                # constant
    x[5, 3] = np.nan
    tab = R.table(x, y, cov, None, "logit")
    assert list(tab[:, 7] < 0) == [False, False, True, True] and np.all(tab[2:, 7] == -2)
    assert np.all(R.table(x, y * 2, cov, None, "logit")[:, 7] == -2)          # a target outside {0, 1}
    assert np.all(R.table(x, np.ones_like(y), cov, None, "logit")[:, 7] == -2)  # one class
    assert np.all(R.table(x[:3], y[:3], cov[:3], None, "ols")[:, 7] == -2)    # n <= P
    assert np.all(R.table(x, y, x[:, :1], None, "ols")[[0], 7] == -2)         # the covariate is the column: singular


@pytest.mark.parametrize("df", [1, 2, 5, 30, 1062, 8190])
def test_student_t_tail_of_the_library(lib, df):
    ts = np.concatenate([np.linspace(0.0, 38.0, 153), [1e-8, 1e-3, 0.5, 1.96, 2.5758]])
    worst = 0.0
    for t in ts:
        want = 2.0 * stats.t.sf(abs(t), df)
        got = lib.nm_student_t_two_sided(float(t), float(df))
        assert want > 0
        worst = max(worst, abs(got - want) / want)
        assert lib.nm_student_t_two_sided(float(-t), float(df)) == got
    print("df", df, "worst relative error", worst)
    assert worst <= 1e-9
    assert np.isnan(lib.nm_student_t_two_sided(float("nan"), float(df)))
    assert lib.nm_student_t_two_sided(float("inf"), float(df)) == 0.0
    assert np.isnan(lib.nm_student_t_two_sided(1.0, 0.0))
