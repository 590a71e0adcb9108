"""The command line of `cnn eval|evalnoise|evalrand --saliency [--saliency-bands N]` (no GPU needed): parsing, what main() refuses,
and what it hands down."""
import pytest

from f2cnn_amd import cli
from f2cnn_amd.scripts.CNN import Evaluating


def parse(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_the_flag_is_absent_unless_given():
    for command in ("eval", "evalnoise", "evalrand"):
        args = parse("cnn", command, "-f", "X.WAV")
        assert "saliency" not in vars(args) and "saliency_bands" not in vars(args)
        assert parse("cnn", command, "-f", "X.WAV", "--saliency").saliency is True
        assert parse("cnn", command, "--saliency", "-f", "X.WAV").file == "X.WAV"
    args = parse("cnn", "eval", "-f", "X.WAV", "--saliency", "--saliency-bands", "16", "--figure-width", "300")
    assert args.saliency is True and args.saliency_bands == 16 and args.figure_width == 300


@pytest.mark.parametrize("bad", ["x", "8.5", "8:8", ""])
def test_bad_band_counts_are_rejected(bad, capsys):
    with pytest.raises(SystemExit):
        parse("cnn", "eval", "-f", "X.WAV", "--saliency", "--saliency-bands=" + bad)
    with pytest.raises(SystemExit):
        parse("cnn", "eval", "-f", "X.WAV", "--saliency=3")          # the flag takes no value
    capsys.readouterr()


def test_what_main_refuses(capsys, monkeypatch):
    called = []
    for name in ("EvaluateOneWavFile", "EvaluateWithNoise", "EvaluateRandom", "EvaluateNoiseSweep", "EvaluateCutoffSweep",
                 "EvaluateReverbSweep", "EvaluateSmearSweep"):
        monkeypatch.setattr(Evaluating, name, lambda *a, _n=name, **kw: called.append(_n))
    for command in ("eval", "evalnoise", "evalrand"):
        assert cli.main(["cnn", command, "-f", "X.WAV", "--saliency", "--occlusion"]) == 1
        assert "one of them" in capsys.readouterr().out
        assert cli.main(["cnn", command, "-f", "X.WAV", "--occlusion", "16:8", "--saliency", "--saliency-bands", "4"]) == 1
        capsys.readouterr()
    for sweep in (["noisesweep", "--snrs", "3"], ["lpfsweep", "--cutoffs", "50"], ["reverbsweep", "--t60", "0.4"], ["smearsweep", "--bands", "8"]):
        assert cli.main(["cnn", sweep[0], "-f", "X.WAV"] + sweep[1:] + ["--saliency"]) == 1
        out = capsys.readouterr().out
        assert "--saliency is not supported by " + sweep[0] in out
    assert cli.main(["cnn", "eval", "-f", "X.WAV", "--saliency-bands", "4"]) == 1
    assert "belongs to --saliency" in capsys.readouterr().out
    assert cli.main(["cnn", "eval", "-f", "X.WAV", "--saliency", "--saliency-bands", "0"]) == 1
    assert "at least 1" in capsys.readouterr().out
    assert not called


def test_main_hands_the_flags_down(monkeypatch):
    seen = {}
    monkeypatch.setattr(Evaluating, "EvaluateOneWavFile", lambda **kw: seen.update(kw))
    assert not cli.main(["cnn", "eval", "-f", "X.WAV", "--saliency", "--figure-width", "300"])
    assert seen["saliency"] == 8 and seen["figure_width"] == 300 and "figure" not in seen and "occlusion" not in seen
    seen.clear()
    assert not cli.main(["cnn", "eval", "-f", "X.WAV", "--saliency", "--saliency-bands", "1", "--hop", "160", "--figure"])
    assert seen["saliency"] == 1 and seen["hop"] == 160 and seen["figure"] is True
    seen.clear()
    assert not cli.main(["cnn", "eval", "-f", "X.WAV"])
    assert "saliency" not in seen and "figure_width" not in seen
    monkeypatch.setattr(Evaluating, "EvaluateWithNoise", lambda **kw: seen.update(kw))
    assert not cli.main(["cnn", "evalnoise", "-f", "X.WAV", "-n", "3", "--saliency"])
    assert seen["saliency"] == 8 and seen["SNRdB"] == 3
    seen.clear()
    monkeypatch.setattr(Evaluating, "EvaluateRandom", lambda **kw: seen.update(kw))
    assert not cli.main(["cnn", "evalrand", "--saliency", "--saliency-bands", "32"])
    assert seen["saliency"] == 32


def test_the_evaluation_functions_refuse_two_maps():
    import numpy as np
    for bad in (dict(saliency=True, occlusion=True), dict(saliency=4, occlusion=(8, 8))):
        with pytest.raises(ValueError):
            Evaluating.EvaluateWavArrays([np.zeros(4000, np.int16)], 16000, model=object(), **bad)
    with pytest.raises(ValueError):
        Evaluating._saliency_bands(0)
    assert Evaluating._saliency_bands(True) == 8 and Evaluating._saliency_bands(3) == 3
