"""`cnn train --engine torch|hip` on the host side: the flag, its default, what is refused, and that the hip engine has no quiet
fall-back. No GPU."""
import numpy as np
import pytest

from f2cnn_amd import _lib, cli
from f2cnn_amd.scripts.CNN import Training


def test_engine_flag_parses_and_is_absent_unless_given():
    p = cli.build_parser()
    assert p.parse_args(["cnn", "train", "--engine", "hip"]).engine == "hip"
    assert p.parse_args(["cnn", "train", "--engine", "torch"]).engine == "torch"
    assert "engine" not in vars(p.parse_args(["cnn", "train"]))        # (the other commands parse as before)
    with pytest.raises(SystemExit):
        p.parse_args(["cnn", "train", "--engine", "keras"])


@pytest.mark.parametrize("argv, want", ((["cnn", "train"], "torch"), (["cnn", "train", "--engine", "torch"], "torch"),
                                        (["cnn", "train", "--engine", "hip"], "hip")))
def test_main_hands_the_engine_to_training(tmp_path, monkeypatch, argv, want):
    monkeypatch.chdir(tmp_path)
    (tmp_path / "trainingData").mkdir()
    (tmp_path / "trainingData" / "last_input_data.npy").write_bytes(b"")
    (tmp_path / "trainingData" / "label_data.csv").write_text("")
    seen = {}
    monkeypatch.setattr(Training, "TrainAndPlotLoss", lambda **kw: seen.update(kw))
    assert cli.main(argv) == 0
    assert seen["engine"] == want


def test_train_and_plot_loss_passes_the_engine_on(tmp_path, monkeypatch):
    from test_training import write_training_set
    monkeypatch.chdir(tmp_path)
    write_training_set(str(tmp_path), n_train=8, n_test=4)
    seen = {}

    def fake_train(*args, **kw):
        seen.update(kw)
        raise KeyboardInterrupt

    monkeypatch.setattr(Training, "normalizeInputBatch", lambda w: np.asarray(w, np.float32))
    monkeypatch.setattr(Training, "train_network", fake_train)
    for engine in Training.ENGINES:
        with pytest.raises(KeyboardInterrupt):
            Training.TrainAndPlotLoss(engine=engine)
        assert seen["engine"] == engine


def test_unknown_engine_is_refused():
    x = np.zeros((4, 11, 128), np.float32)
    with pytest.raises(ValueError, match="engine"):
        Training.train_network(x, np.zeros(4), x, np.zeros(4), epochs=1, device="cpu", engine="keras")
    assert Training.ENGINES == ("torch", "hip")


def test_hip_engine_without_a_device_raises(monkeypatch):
    """no library or no device: the error of the context reaches the caller, and nothing trains in its place"""
    def no_device(device=None):
        raise _lib.F2Error(_lib.F2_ERR_HIP, "no HIP device available")

    monkeypatch.setattr(_lib, "default_context", no_device)
    monkeypatch.setattr(Training, "_torch_engine", lambda *a, **k: pytest.fail("the hip engine fell back to torch"))
    x = np.zeros((4, 11, 128), np.float32)
    with pytest.raises(_lib.F2Error):
        Training.train_network(x, np.zeros(4), x, np.zeros(4), epochs=1, engine="hip")
    with pytest.raises(_lib.F2Error):                  # device="cpu" overrides the torch engine's check only: no fall-back
        Training.train_network(x, np.zeros(4), x, np.zeros(4), epochs=1, device="cpu", engine="hip")


def test_usage_text_names_the_flag():
    assert "--engine torch|hip" in cli.__doc__
    sub = [a for a in cli.build_parser()._subparsers._group_actions[0].choices["cnn"]._actions if "--engine" in a.option_strings]
    assert len(sub) == 1 and tuple(sub[0].choices) == ("torch", "hip")
