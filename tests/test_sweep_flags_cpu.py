"""The refusals of the `test` subcommand and of the library functions behind it (CPU): every flag that needs another one, every
value out of range and every malformed TARGET:KIND leaves through the parser with exit code 2 and its own message, before a
cohort is built or a GPU is asked for; where two rules are broken, the one that comes first in the parser's order is reported."""
import pytest

from multi_modal_normative_modeling_amd import _lib, metrics, sweep

ROI = ["--roi-effect"]
CENT = ROI + ["--centile", "signed"]
NORM = ROI + ["--normative", "signed"]
MAHA = ["--latent", "--mahalanobis"]
TAIL = "--tail must lie inside (0, 50)"
QUANT = f"--quantiles: at most {_lib.NM_CENT_MAX_Q} probabilities inside [0, 1]"
Z_THR = "--z-thr must be finite and > 0"
RIDGE = "--ridge must be finite and >= 0"


def _spec_message(spec):
    return (f"a TARGET:KIND pair is needed, TARGET one of {sorted(sweep.REGRESS_TARGETS)} and KIND one of "
            f"{sorted(metrics.COLUMN_REGRESS_KINDS)}; got {spec!r}")


REFUSED = [
    # X needs Y
    (["--centile", "squared"], "--centile needs --roi-effect"),
    (["--normative", "squared"], "--normative needs --roi-effect"),
    (["--roi-significance"], "--roi-significance needs --roi-effect"),
    (["--roi-regress", "DIA:logit"], "--roi-regress needs --roi-effect"),
    (ROI + ["--centile-loo"], "--centile-loo needs --centile"),
    (ROI + ["--robust"], "--robust needs --normative"),
    (["--mahalanobis"], "--mahalanobis needs --latent"),
    (["--latent-pvalues", "DIA:logit"], "--latent-pvalues needs --latent"),
    (ROI + ["--roi-adjust", "AGE"], "--roi-adjust needs --roi-regress"),
    # ranges
    (CENT + ["--tail", "0"], TAIL),
    (CENT + ["--tail", "50"], TAIL),
    (CENT + ["--tail", "nan"], TAIL),
    (CENT + ["--quantiles", "0.5", "1.5"], QUANT),
    (CENT + ["--quantiles", "-0.1"], QUANT),
    (CENT + ["--quantiles"] + ["0.5"] * (_lib.NM_CENT_MAX_Q + 1), QUANT),
    (NORM + ["--z-thr", "0"], Z_THR),
    (NORM + ["--z-thr", "nan"], Z_THR),
    (MAHA + ["--ridge", "-1"], RIDGE),
    (MAHA + ["--ridge", "nan"], RIDGE),
    # TARGET:KIND
    (ROI + ["--roi-regress", "DIA"], _spec_message("DIA")),
    (ROI + ["--roi-regress", "DIA:probit"], _spec_message("DIA:probit")),
    (["--latent", "--latent-pvalues", "AGE:ols", "HEIGHT:ols"], _spec_message("HEIGHT:ols")),
    # two at once: the parser's order decides, not the order on the command line
    (["--robust", "--centile", "signed"], "--centile needs --roi-effect"),
    (["--roi-significance", "--mahalanobis"], "--mahalanobis needs --latent"),
    (ROI + ["--roi-adjust", "AGE", "--normative", "signed", "--z-thr", "0", "--centile-loo"], "--centile-loo needs --centile"),
    (CENT + ["--quantiles", "2", "--tail", "0"], TAIL),
    (ROI + ["--roi-regress", "DIA", "--latent", "--latent-pvalues", "AGE"], _spec_message("AGE")),
    (["--latent", "--latent-pvalues", "AGE", "--roi-adjust", "AGE"], "--roi-adjust needs --roi-regress"),
]


@pytest.mark.parametrize("argv, message", REFUSED, ids=[" ".join(a)[:60] for a, _ in REFUSED])
def test_the_test_subcommand_refuses(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        sweep.main_test(["--models-dir", "nowhere"] + argv)
    assert e.value.code == 2
    assert capsys.readouterr().err.rstrip("\n").endswith(" test: error: " + message)


def test_values_of_a_switched_off_statistic_are_not_judged(capsys):
    # (the range rules belong to their switch: without it the value is never used.  The run gets past the parser and ends at the
    #  unknown dataset, the first thing after it)
    for argv in (["--tail", "0"], ["--quantiles", "2"], ["--z-thr", "nan"], ["--ridge", "-1"]):
        with pytest.raises(ValueError, match="Unknown dataset"):
            sweep.main_test(["--models-dir", "nowhere", "-R", "nowhere"] + argv)


@pytest.mark.parametrize("kw", [dict(roi_significance=True), dict(roi_regress=("logit", "DIA")), dict(robust=True)],
                         ids=["roi_significance", "roi_regress", "robust"])
def test_test_folds_refuses_a_statistic_without_its_prerequisite(kw):
    with pytest.raises(ValueError, match="needs"):
        sweep.test_folds([], None, [], ["a"], "poe", "cpu", **kw)
