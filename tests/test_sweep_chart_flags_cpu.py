"""The refusals around `test --trajectory-fold` and test_folds(trajectory_fold=...) (CPU): the flag needs --trajectory, takes
"export" or "kernel" and nothing else, and leaves through the parser with exit code 2 before a cohort is built."""
import pytest

from multi_modal_normative_modeling_amd import sweep


def test_the_names_of_the_folds():
    assert sweep.TRAJ_FOLDS == ("export", "kernel")
    assert (sweep.TRAJ_MIN_ROWS, sweep.TRAJ_MAX_ROWS) == (16, 4096)
    assert sweep.check_trajectory_fold(None, None) == "export" and sweep.check_trajectory_fold(None, 32) == "export"
    assert sweep.check_trajectory_fold("kernel", 32) == "kernel" and sweep.check_trajectory_fold("export", 32) == "export"
    with pytest.raises(ValueError, match="trajectory_fold must be one of"):
        sweep.check_trajectory_fold("device", 32)
    with pytest.raises(ValueError, match="trajectory_fold needs trajectory"):
        sweep.check_trajectory_fold("kernel", None)


@pytest.mark.parametrize("argv, message", [
    (["--trajectory-fold", "kernel"], "--trajectory-fold needs --trajectory"),
    (["--trajectory-fold", "export"], "--trajectory-fold needs --trajectory"),
    (["--trajectory-fold", "kernel", "--traj-seed", "3"], "--traj-seed needs --trajectory"),          # the parser's order decides
    (["--trajectory", "40", "--trajectory-fold", "kernel"], "--trajectory must be a multiple of 16 from 16 to 4096"),
])
def test_the_test_subcommand_refuses(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        sweep.main_test(["--models-dir", "nowhere"] + argv)
    assert e.value.code == 2
    assert capsys.readouterr().err.rstrip("\n").endswith(" test: error: " + message)


def test_an_unknown_fold_is_an_argument_error(capsys):
    with pytest.raises(SystemExit) as e:
        sweep.main_test(["--models-dir", "nowhere", "--trajectory", "32", "--trajectory-fold", "device"])
    assert e.value.code == 2
    assert "--trajectory-fold" in capsys.readouterr().err


def test_a_valid_pair_gets_past_the_parser():
    with pytest.raises(ValueError, match="Unknown dataset"):          # the first thing after the parser
        sweep.main_test(["--models-dir", "nowhere", "-R", "nowhere", "--trajectory", "32", "--trajectory-fold", "kernel"])


def test_test_folds_refuses_a_fold_without_trajectory():
    with pytest.raises(ValueError, match="trajectory_fold needs trajectory"):
        sweep.test_folds([], None, [], ["a"], "poe", "cpu", trajectory_fold="kernel")
    with pytest.raises(ValueError, match="trajectory_fold must be one of"):
        sweep.test_folds([], None, [], ["a"], "poe", "cpu", trajectory=32, trajectory_fold="device")
