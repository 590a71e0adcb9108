"""CPU-only checks of `prepare input --from-wav`: the flag parses, belongs to `prepare input` alone, and the label keys
map to the audio files."""
import os

import pytest

from f2cnn_amd import cli


def test_parser_accepts_from_wav():
    a = cli.build_parser().parse_args(["prepare", "input", "--from-wav", "--cutoff", "50", "--metrics", "m.json"])
    assert a.from_wav and a.CUTOFF == 50 and a.metrics == "m.json" and a.prepare_command == "input"
    assert not cli.build_parser().parse_args(["prepare", "input"]).from_wav


@pytest.mark.parametrize("command", ["filter", "envelope", "label", "features"])
def test_from_wav_with_another_prepare_command_fails(command, capsys):
    assert cli.main(["prepare", command, "--from-wav"]) == 1
    assert "--from-wav" in capsys.readouterr().out


def test_label_key_to_wav():
    from f2cnn_amd.scripts.processing.InputGenerator import wav_for_label_key
    assert wav_for_label_key(os.path.join("TRAIN", "DR1.FCJF0.SA1.ENV1.npy")) == \
        os.path.join("resources", "f2cnn", "TRAIN", "DR1.FCJF0.SA1.WAV")
