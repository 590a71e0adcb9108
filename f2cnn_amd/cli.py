"""Command line of the hot path, same surface as the reference's f2cnn.py (:68-160) for the commands this
package implements:

    python -m f2cnn_amd prepare filter
    python -m f2cnn_amd prepare envelope [--cutoff/-c HZ]
    python -m f2cnn_amd prepare label                       (needs the VTR .FB and TIMIT .PHN side files)
    python -m f2cnn_amd prepare input [--cutoff HZ] [--label/-l CSV] [--input/-i NPY]
    python -m f2cnn_amd prepare input --from-wav [--cutoff HZ] [--label/-l CSV] [--input/-i NPY] [--metrics FILE]
                                                            (windows straight from the WAV files: no .GFB.npy / .ENV1.npy
                                                             on disk; --cutoff low-passes the envelopes; not in the reference)
    python -m f2cnn_amd prepare features [--cutoff HZ]     (filter + envelope in one pass, not in the reference)
    (filter / envelope / features also take --skip-existing to resume and --metrics FILE for a JSON summary; a file that
     cannot be read is reported and skipped, the exit status is then 2)
    python -m f2cnn_amd cnn train [--input/-i NPY] [--label/-l CSV] [--engine torch|hip]
                                                            (weights -> last_trained_model; --engine torch, the default: PyTorch-ROCm
                                                             autograd; --engine hip: the library's own training step - weight
                                                             gradients, dropout and RMSprop on the device, the same seed giving the
                                                             same weights bit for bit)
    python -m f2cnn_amd cnn train --engine hip --from-wav [--lpf HZ] [--augment-snrs 20,10,5,0] [--seed S] [--label/-l CSV]
                                                            (training windows rendered on the device from the WAV files of the
                                                             label CSV's TRAIN rows, no input .npy; with --augment-snrs they are
                                                             rendered again before every epoch, every file at a level drawn from
                                                             the list or clean under fresh white noise, and the TEST files are
                                                             validated clean and at every level; --engine torch cannot do either;
                                                             not in the reference)
    python -m f2cnn_amd cnn train --engine hip --from-wav [--augment-t60 0.2,0.4,0.8] [--augment-rirs a.wav,b.wav] [--drr DB] [--augment-snrs ...] [--seed S]
                                                            (every epoch each TRAIN file is also convolved on the device with the
                                                             response of a room drawn from the list - synthetic ones built anew
                                                             every epoch, measured ones fixed - or left dry; room first, then
                                                             noise at an SNR of the reverberant signal; the TEST files are also
                                                             validated once per room; not in the reference)
    python -m f2cnn_amd cnn train --engine hip --from-wav --augment-snrs 20,10 --augment-colours white,pink,speech,like:babble.wav [--augment-noise-taps N] [--seed S]
                                                            (a noise level is a pair (colour, SNR), colour-major over the SNRs as
                                                             in noisesweep --colours, at most 64: every epoch each TRAIN file is
                                                             rendered under one of them or clean, the noise filtered on the
                                                             device; the TEST files are validated once per pair; needs
                                                             --augment-snrs; not in the reference)
    python -m f2cnn_amd cnn train --engine hip --from-wav [--augment-spreads 0.5,1,2,4] [--augment-bands 16,8] [--augment-snrs ...] [--augment-t60 ...] [--seed S]
                                                            (every epoch each TRAIN file is also rendered at a spectral resolution
                                                             drawn from the levels of smearsweep - channel interaction of that
                                                             many ERB, then N-band vocoders - or sharp: the envelopes of its
                                                             windows are mixed across the channels on the device, in the gather,
                                                             before they are normalised; the TEST files are also validated once
                                                             per resolution; combines with every other --augment option; not in
                                                             the reference)
    python -m f2cnn_amd cnn train --engine hip --from-wav --augment-maskers babble.wav,cafe.wav --augment-masker-snrs 20,10,5 [--augment-snrs ...] [--seed S]
                                                            (a masker level is a pair (recording, SNR), masker-major over the SNRs
                                                             as in noisesweep --maskers, at most 64: every epoch each TRAIN file is
                                                             rendered under a segment of one of the recordings or without, mixed
                                                             on the device behind the room and before the Gaussian noise; the
                                                             TEST files are validated once per pair; combines with every other
                                                             --augment option; not in the reference)
    python -m f2cnn_amd cnn train --engine hip --from-wav --augment-cutoffs 5,10,20,50 [--augment-snrs ...] [--augment-t60 ...] [--seed S]
                                                            (every epoch the envelopes of each TRAIN file are low-passed at a
                                                             cutoff drawn from the levels of lpfsweep, at most 64, or left
                                                             unfiltered: filtered on the device between the envelopes and the
                                                             gather; the TEST files are also validated once per cutoff; not with
                                                             --lpf; combines with every other --augment option; not in the
                                                             reference)
    python -m f2cnn_amd cnn test [--input/-i NPY] [--label/-l CSV] [--model/-m NPZ] [--by set|region|speaker|phoneme] [--rows test|train|all]
                                                            (loss, accuracy and the 2 x 2 counts of a saved model on the labelled
                                                             windows, per value of a label column, in one device pass; writes
                                                             <model>_test.json, a trailing .npz of the name dropped; the
                                                             reference only scores right after training)
    python -m f2cnn_amd cnn eval --file/-f WAV [--lpf HZ] [--model/-m NPZ] [--hop N|frame]
    python -m f2cnn_amd cnn evalnoise --file/-f WAV --noise/-n SNRdB [--lpf HZ] [--model/-m NPZ] [--hop N|frame]
    python -m f2cnn_amd cnn noisesweep --file/-f WAV --snrs 20,10,0,-3 [--seed N] [--save-wavs] [--hop N|frame] [--lpf HZ] [--model/-m NPZ]
                                                            (the file at every level and clean in one device pass, agreement
                                                             with the clean decisions per level; not in the reference)
    python -m f2cnn_amd cnn noisesweep --file/-f WAV --snrs 20,10,0 --colours white,pink,speech,like:babble.wav,fir:taps.npy [--noise-taps N] [--seed N] [--hop N|frame] [--lpf HZ] [--accuracy [MODE]] [--resample] [--save-wavs]
                                                            (the same under coloured noise: every colour at every level, colour-
                                                             major, at most 64 levels, in one device pass - Gaussian noise through
                                                             a filter of N taps (default 1025, odd) with the long-term spectrum of
                                                             pink or brown noise, of speech, of a mono recording at the file's rate
                                                             (like:) or of taps of one's own (fir:), scaled so that an SNR means
                                                             what it means for white noise; levels are named like `pink 10dB`,
                                                             written to OutputWavFiles/addedNoise/<stem>.coloursweep.npz; --colours
                                                             and --noise-taps are refused on every other command; not in the
                                                             reference)
    python -m f2cnn_amd cnn noisesweep --file/-f WAV --snrs 20,10,0 --maskers babble.wav,cafe.wav [--seed N] [--hop N|frame] [--lpf HZ] [--accuracy [MODE]] [--resample] [--save-wavs]
                                                            (the same under recorded maskers: a cyclic segment of every recording,
                                                             drawn per file from the seed, scaled to every level and mixed in on
                                                             the device - the recording itself with its own modulations, not a
                                                             Gaussian noise of its spectrum; masker-major, at most 64 levels named
                                                             like `babble 10dB`, written to
                                                             OutputWavFiles/addedNoise/<stem>.maskersweep.npz; a recording at
                                                             another rate needs --resample; not together with --colours; not in
                                                             the reference)
    python -m f2cnn_amd cnn lpfsweep --file/-f WAV --cutoffs 5,10,20,50,100 [--hop N|frame] [--accuracy [MODE]] [--resample] [--model/-m NPZ]
                                                            (the file at every envelope cutoff and unfiltered in one device pass -
                                                             filterbank and Hilbert envelope run once - agreement with the
                                                             unfiltered decisions per cutoff, written to <base>.lpfsweep.npz; takes
                                                             no --lpf, --figure, --occlusion or --saliency; not in the reference)
    python -m f2cnn_amd cnn reverbsweep --file/-f WAV --t60 0.2,0.4,0.8 [--rir room.wav[,hall.wav]] [--drr DB] [--seed N] [--save-wavs] [--hop N|frame] [--lpf HZ] [--accuracy [MODE]] [--resample] [--model/-m NPZ]
                                                            (the file in every room and dry in one device pass - synthetic
                                                             responses of the given reverberation times in seconds, direct-to-
                                                             reverberant ratio DB (default 0), and / or measured ones from mono
                                                             WAV files at the file's rate - agreement with the dry decisions per
                                                             level, written to OutputWavFiles/reverb/<stem>.reverbsweep.npz; takes
                                                             no --figure or --occlusion; not in the reference)
    python -m f2cnn_amd cnn smearsweep --file/-f WAV [--spreads 0.5,1,2,4] [--bands 32,16,8] [--hop N|frame] [--lpf HZ] [--accuracy [MODE]] [--resample] [--model/-m NPZ]
                                                            (the file at every spectral resolution and sharp in one device pass -
                                                             filterbank and envelope run once; --spreads: channel interaction, a
                                                             Gaussian spread in ERB across the channels' envelopes; --bands: an
                                                             N-band vocoder, every channel replaced by the mean of its band; at
                                                             least one of the two - agreement with the sharp decisions per level,
                                                             written to <base>.smearsweep.npz; takes no --figure or --occlusion;
                                                             not in the reference)
    python -m f2cnn_amd cnn evalrand [--count/-c N] [--lpf HZ] [--model/-m NPZ] [--hop N|frame]
    (--hop: a decision every N samples instead of every sample, `frame` = one per STEP of configF2CNN.conf; not in the reference)
    (eval / evalnoise / evalrand / noisesweep also take --accuracy [reference|centre]: the decisions against the labels of the
     source file's .FB / .PHN, as the reference's EvaluateOneWavArray ends - per file, per noise level, and for evalrand over
     the corpus. `reference`, also the bare flag, compares the row index times the hop with the label timepoint as the
     reference does; `centre` compares the row's centre sample, RADIUS * STEP further on)
    (eval / evalnoise / evalrand / noisesweep also take --resample: every file is brought to FRAMERATE of configF2CNN.conf and to
     one channel on the device before anything else sees it - any sample rate, 8 / 16 / 24 / 32-bit integer and float RIFF files,
     the channels of a stereo file averaged - with scipy.signal.resample_poly's filter; STEP and `--hop frame` are then those of
     FRAMERATE, and the .npz files also hold framerate and source_framerate. Without it a file is evaluated at its own rate, as
     the reference does; not in the reference)
    (eval / evalnoise / evalrand also take --figure [--figure-width W]: the figure the reference's EvaluateOneWavArray ends in -
     the gammatonegram with the formant track and a rising / falling tick per decision, below it the network's probability of
     "rising" beside arctan of the formant's slope, its p-value and the phoneme boundaries - as
     graphs/FallingOrRising/<basename>.png, W (default 1600) columns wide, without matplotlib; decisions and picture come from
     one device pass and the .npz also holds figure_track and figure_span)
    (eval / evalnoise / evalrand also take --occlusion [BAND[:STRIDE]] [--occlusion-rows RBAND[:RSTRIDE]] [--occlusion-fill V]:
     the occlusion map - every window evaluated again with each band of channels blanked, in the same device pass; one table
     line per band (Hz range, rows, flips, mean change of P(rising)), graphs/Occlusion/<basename>.png with the map under the
     gammatonegram, --figure-width columns wide, and occlusion_* keys in the .npz; scores and labels stay those without the
     flag; not in the reference)
    (eval / evalnoise / evalrand also take --saliency [--saliency-bands N]: the saliency map - the gradient of P(rising) at every
     cell of every normalised window from one backward pass on the device, whatever the resolution; one table line per N channels
     (default 8: Hz range, rows, sum of the mean G x, sum of the mean |G|; the G x column reads against --occlusion 8:8 with the sign
     reversed), graphs/Saliency/<basename>.png with the G x map under the gammatonegram, --figure-width columns wide, and
     saliency_map, saliency_summary, saliency_span in the .npz; scores and labels stay those without the flag; one map per run,
     so not together with --occlusion, and not on the sweeps; not in the reference)
    (eval / evalnoise / evalrand also take --segments [--dwell MS] [--segments-weight auto|X]: the decisions smoothed into
     transitions - the most probable rising / falling sequence of a two-state chain whose states last MS on average (default
     three label frames, 30 ms at 16 kHz: a default, not a tuned value), decoded on the device in the same pass; one table line
     per run (start, end, duration, decision, mean log-odds, the phonemes it overlaps), with the file's .PHN a second table per
     phoneme (rows, % rising raw and smoothed, mean log-odds), and segments_* keys in the .npz; with --accuracy a second accuracy
     line for the smoothed decisions; scores and labels stay those without the flag; not on the sweeps; not in the reference)
    python -m f2cnn_amd plot gtg [--file/-f WAV | --all] [--width W] [--pool mean|max] [--cutoff HZ] [--formant N] [--start S --end E] [--out PNG]
                                                            (gammatonegram pictures, pooled to W columns and log-normalised on the
                                                             device, written as graphs/gtg/<basename>.png without matplotlib; the
                                                             VTR formant tracks on top when the .FB is there; --all takes
                                                             resources/f2cnn/*/*.WAV; S and E are sample indices)
    python -m f2cnn_amd --configure            (writes configF2CNN.conf with the reference's defaults)

organize needs the licensed TIMIT+VTR corpora and stays with the reference.
"""
import argparse

PREPARE = ("filter", "envelope", "label", "input", "features")
CNN = ("train", "test", "eval", "evalnoise", "evalrand", "noisesweep", "lpfsweep", "reverbsweep", "smearsweep")
PLOT = ("gtg",)


def hop_argument(text):
    """--hop: a positive number of samples, or 'frame' (resolved to STEP once the configuration is read)"""
    if text == 'frame':
        return text
    try:
        hop = int(text)
    except ValueError:
        hop = 0
    if hop < 1:
        raise argparse.ArgumentTypeError("--hop takes a positive number of samples or 'frame', not {!r}".format(text))
    return hop


def snrs_argument(text):
    """--snrs: a comma-separated list of at least one finite SNR in dB"""
    import math
    try:
        snrs = [float(part) for part in text.split(',')]
    except ValueError:
        snrs = []
    if not snrs or not all(math.isfinite(v) for v in snrs):
        raise argparse.ArgumentTypeError("--snrs takes a comma-separated list of SNRs in dB, not {!r}".format(text))
    return snrs


def augment_snrs_argument(text):
    """--augment-snrs: as --snrs"""
    try:
        return snrs_argument(text)
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError("--augment-snrs takes a comma-separated list of SNRs in dB, not {!r}".format(text))


def augment_t60_argument(text):
    """--augment-t60: as --t60"""
    try:
        return t60_argument(text)
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError("--augment-t60 takes a comma-separated list of positive reverberation times in seconds, not {!r}"
                                         .format(text))


def augment_rirs_argument(text):
    """--augment-rirs: as --rir"""
    try:
        return rir_argument(text)
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError("--augment-rirs takes a comma-separated list of WAV files, not {!r}".format(text))


def cutoffs_argument(text):
    """--cutoffs: a comma-separated list of at least one finite cutoff in (0, 8000) Hz"""
    import math
    try:
        cutoffs = [float(part) for part in text.split(',')]
    except ValueError:
        cutoffs = []
    if not cutoffs or not all(math.isfinite(v) and 0 < v < 8000 for v in cutoffs):
        raise argparse.ArgumentTypeError("--cutoffs takes a comma-separated list of cutoffs in Hz inside (0, 8000), not {!r}".format(text))
    return cutoffs


def augment_cutoffs_argument(text):
    """--augment-cutoffs: as --cutoffs, at most NOISE_LEVELS_MAX"""
    try:
        cutoffs = cutoffs_argument(text)
    except argparse.ArgumentTypeError as e:
        raise argparse.ArgumentTypeError(str(e).replace('--cutoffs', '--augment-cutoffs'))
    if len(cutoffs) > NOISE_LEVELS_MAX:
        raise argparse.ArgumentTypeError("--augment-cutoffs takes at most {} cutoffs, not {}".format(NOISE_LEVELS_MAX, len(cutoffs)))
    return cutoffs


def t60_argument(text):
    """--t60: a comma-separated list of at least one finite, positive reverberation time in seconds"""
    import math
    try:
        t60s = [float(part) for part in text.split(',')]
    except ValueError:
        t60s = []
    if not t60s or not all(math.isfinite(v) and v > 0 for v in t60s):
        raise argparse.ArgumentTypeError("--t60 takes a comma-separated list of positive reverberation times in seconds, not {!r}".format(text))
    return t60s


def spreads_argument(text):
    """--spreads: a comma-separated list of at least one finite, positive spread in ERB"""
    import math
    try:
        spreads = [float(part) for part in text.split(',')]
    except ValueError:
        spreads = []
    if not spreads or not all(math.isfinite(v) and v > 0 for v in spreads):
        raise argparse.ArgumentTypeError("--spreads takes a comma-separated list of positive spreads in ERB, not {!r}".format(text))
    return spreads


def bands_argument(text):
    """--bands: a comma-separated list of at least one positive whole number of bands"""
    try:
        bands = [int(part) for part in text.split(',')]
    except ValueError:
        bands = []
    if not bands or not all(v >= 1 for v in bands):
        raise argparse.ArgumentTypeError("--bands takes a comma-separated list of positive whole numbers of bands, not {!r}".format(text))
    return bands


def rir_argument(text):
    """--rir: a comma-separated list of at least one impulse response file"""
    files = text.split(',')
    if not all(files):
        raise argparse.ArgumentTypeError("--rir takes a comma-separated list of WAV files, not {!r}".format(text))
    return files


def drr_argument(text):
    """--drr: a finite direct-to-reverberant ratio in dB"""
    import math
    try:
        drr = float(text)
    except ValueError:
        drr = math.nan
    if not math.isfinite(drr):
        raise argparse.ArgumentTypeError("--drr takes a direct-to-reverberant ratio in dB, not {!r}".format(text))
    return drr


NOISE_COLOURS = ('white', 'pink', 'brown', 'speech')     # noise.COLOURS (kept here so that parsing imports nothing)
NOISE_LEVELS_MAX = 64
SMEAR_LEVELS_MAX = 64                                    # F2_SMEAR_MAX_LEVELS (likewise)
MASKER_RECORDINGS_MAX = 64                               # F2_MASKER_MAX_RECORDINGS (likewise; the levels: NOISE_LEVELS_MAX)


def colours_argument(text):
    """--colours: a comma-separated list of at least one colour - a name of NOISE_COLOURS, like:<recording.wav> or fir:<taps.npy>"""
    colours = text.split(',')
    for c in colours:
        named = c.split(':', 1)
        if not (c in NOISE_COLOURS or (len(named) == 2 and named[0] in ('like', 'fir') and named[1])):
            raise argparse.ArgumentTypeError("--colours takes a comma-separated list of {}, like:<recording.wav> or fir:<taps.npy>, "
                                             "not {!r}".format(', '.join(NOISE_COLOURS), text))
    return colours


def noise_taps_argument(text):
    """--noise-taps: an odd, positive number of filter taps (the library's limit is checked where the filters are built)"""
    try:
        taps = int(text)
    except ValueError:
        taps = 0
    if taps < 1 or taps % 2 == 0:
        raise argparse.ArgumentTypeError("--noise-taps takes an odd, positive number of taps, not {!r}".format(text))
    return taps


def augment_colours_argument(text):
    """--augment-colours: as --colours"""
    try:
        return colours_argument(text)
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError("--augment-colours takes a comma-separated list of {}, like:<recording.wav> or "
                                         "fir:<taps.npy>, not {!r}".format(', '.join(NOISE_COLOURS), text))


def augment_noise_taps_argument(text):
    """--augment-noise-taps: as --noise-taps"""
    try:
        return noise_taps_argument(text)
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError("--augment-noise-taps takes an odd, positive number of taps, not {!r}".format(text))


def maskers_argument(text, option='--maskers'):
    """--maskers: a comma-separated list of at least one recording (RIFF files; read where they are used)"""
    maskers = text.split(',')
    if not all(maskers):
        raise argparse.ArgumentTypeError("{} takes a comma-separated list of recordings, not {!r}".format(option, text))
    if len(maskers) > MASKER_RECORDINGS_MAX:
        raise argparse.ArgumentTypeError("{} takes at most {} recordings, not {}".format(option, MASKER_RECORDINGS_MAX, len(maskers)))
    return maskers


def augment_maskers_argument(text):
    """--augment-maskers: as --maskers"""
    return maskers_argument(text, '--augment-maskers')


def augment_masker_snrs_argument(text):
    """--augment-masker-snrs: as --augment-snrs"""
    try:
        return augment_snrs_argument(text)
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError("--augment-masker-snrs takes a comma-separated list of SNRs in dB, not {!r}".format(text))


def build_parser():
    parser = argparse.ArgumentParser(prog="f2cnn_amd", description="F2CNN hot path on MI355X.")
    parser.add_argument('--configure', action='store_true', help='write configF2CNN.conf with default values')
    sub = parser.add_subparsers()
    p = sub.add_parser('prepare', help='data processing commands')
    p.add_argument('--cutoff', '-c', action='store', dest='CUTOFF', type=int,
                   help="low pass filter the envelopes with this cutoff frequency")
    p.add_argument('prepare_command', choices=PREPARE)
    p.add_argument('--file', '-f', dest='file', nargs='?')
    p.add_argument('--input', '-i', dest='inputFile', nargs='?')
    p.add_argument('--label', '-l', dest='labelFile', nargs='?')
    p.add_argument('--skip-existing', action='store_true',
                   help="filter / envelope / features: leave files whose outputs are already up to date (resume)")
    p.add_argument('--metrics', dest='metrics', nargs='?',
                   help="filter / envelope / features / input --from-wav: write files, audio seconds, wall time and "
                        "audio-s/s as JSON")
    p.add_argument('--from-wav', dest='from_wav', action='store_true',
                   help="input: build the windows from the WAV files on the device (envelopes low-passed at --cutoff), "
                        "without .GFB.npy / .ENV1.npy files")
    c = sub.add_parser('cnn', help='CNN commands')
    c.add_argument('--file', '-f', dest='file', nargs='?')
    c.add_argument('--input', '-i', dest='inputFile', nargs='?')
    c.add_argument('--label', '-l', dest='labelFile', nargs='?')
    c.add_argument('--model', '-m', dest='model', nargs='?')
    c.add_argument('cnn_command', choices=CNN)
    c.add_argument('--lpf', action='store', type=int, dest='CUTOFF', help="low pass filter the envelopes")
    c.add_argument('--count', '-c', action='store', type=int, help="number of files to evaluate (evalrand)")
    c.add_argument('--noise', '-n', action='store', type=float, dest='SNRdB', help="SNR in dB (evalnoise)")
    c.add_argument('--hop', action='store', type=hop_argument, dest='hop',
                   help="eval / evalnoise / evalrand: evaluate every HOP-th sample ('frame': every STEP samples) instead of "
                        "every sample")
    c.add_argument('--snrs', action='store', type=snrs_argument, dest='snrs',
                   help="noisesweep: comma-separated SNRs in dB, e.g. 20,10,0,-3")
    # (absent from the parsed arguments unless given: the commands parse as before without it)
    c.add_argument('--cutoffs', action='store', type=cutoffs_argument, dest='cutoffs', default=argparse.SUPPRESS,
                   help="lpfsweep: comma-separated envelope cutoffs in Hz, e.g. 5,10,20,50,100")
    # (absent from the parsed arguments unless given: the commands parse as before without them)
    c.add_argument('--t60', action='store', type=t60_argument, dest='t60', default=argparse.SUPPRESS,
                   help="reverbsweep: comma-separated reverberation times in seconds, e.g. 0.2,0.4,0.8")
    c.add_argument('--rir', action='store', type=rir_argument, dest='rir', default=argparse.SUPPRESS,
                   help="reverbsweep: comma-separated mono WAV files with measured impulse responses at the file's rate")
    c.add_argument('--drr', action='store', type=drr_argument, dest='drr', default=argparse.SUPPRESS,
                   help="reverbsweep: direct-to-reverberant ratio of the synthetic responses in dB (default 0)")
    c.add_argument('--spreads', action='store', type=spreads_argument, dest='spreads', default=argparse.SUPPRESS,
                   help="smearsweep: comma-separated spreads of the channel interaction in ERB, e.g. 0.5,1,2,4")
    c.add_argument('--bands', action='store', type=bands_argument, dest='bands', default=argparse.SUPPRESS,
                   help="smearsweep: comma-separated numbers of vocoder bands, e.g. 32,16,8")
    # (absent from the parsed arguments unless given: the commands parse as before without it)
    c.add_argument('--engine', action='store', dest='engine', choices=('torch', 'hip'), default=argparse.SUPPRESS,
                   help="train: 'torch' (PyTorch-ROCm autograd, the default) or 'hip' (the library's own training step)")
    c.add_argument('--from-wav', action='store_true', dest='from_wav', default=argparse.SUPPRESS,
                   help="train --engine hip: render the training windows from the WAV files on the device (envelopes low-passed at "
                        "--lpf), without an input .npy")
    c.add_argument('--augment-snrs', action='store', type=augment_snrs_argument, dest='augment_snrs', default=argparse.SUPPRESS,
                   help="train --engine hip --from-wav: comma-separated SNRs in dB; every epoch each file is rendered at one of them "
                        "or clean, under fresh noise")
    c.add_argument('--augment-t60', action='store', type=augment_t60_argument, dest='augment_t60', default=argparse.SUPPRESS,
                   help="train --engine hip --from-wav: comma-separated reverberation times in seconds; every epoch each file is "
                        "rendered in a fresh synthetic room of one of them (--drr: their direct-to-reverberant ratio) or dry")
    c.add_argument('--augment-rirs', action='store', type=augment_rirs_argument, dest='augment_rirs', default=argparse.SUPPRESS,
                   help="train --engine hip --from-wav: comma-separated mono WAV files with measured impulse responses, further rooms "
                        "of the draw")
    c.add_argument('--augment-colours', action='store', type=augment_colours_argument, dest='augment_colours', default=argparse.SUPPRESS,
                   help="train --engine hip --from-wav --augment-snrs: comma-separated noise colours, as noisesweep's --colours; every "
                        "epoch each file is rendered under one (colour, SNR) pair or clean")
    c.add_argument('--augment-spreads', action='store', type=spreads_argument, dest='augment_spreads', default=argparse.SUPPRESS,
                   help="train --engine hip --from-wav: comma-separated spreads in ERB, as smearsweep's --spreads; every epoch each "
                        "file is rendered at one of the spectral resolutions, or sharp")
    c.add_argument('--augment-bands', action='store', type=bands_argument, dest='augment_bands', default=argparse.SUPPRESS,
                   help="train --engine hip --from-wav: comma-separated numbers of vocoder bands, as smearsweep's --bands; levels "
                        "behind those of --augment-spreads")
    c.add_argument('--augment-noise-taps', action='store', type=augment_noise_taps_argument, dest='augment_noise_taps',
                   default=argparse.SUPPRESS, help="train --augment-colours: taps of the designed noise filters, odd (default 1025, at most 2047)")
    # (absent from the parsed arguments unless given: the commands parse as before without them)
    c.add_argument('--colours', action='store', type=colours_argument, dest='colours', default=argparse.SUPPRESS,
                   help="noisesweep: comma-separated noise colours - white, pink, brown, speech, like:<recording.wav> (the long-term "
                        "spectrum of a mono recording at the file's rate), fir:<taps.npy> - every one at every level of --snrs")
    c.add_argument('--noise-taps', action='store', type=noise_taps_argument, dest='noise_taps', default=argparse.SUPPRESS,
                   help="noisesweep --colours: taps of the designed noise filters, odd (default 1025, at most 2047)")
    c.add_argument('--maskers', action='store', type=maskers_argument, dest='maskers', default=argparse.SUPPRESS,
                   help="noisesweep: comma-separated recordings (babble, a cafeteria, music; any RIFF at the file's rate, any rate with "
                        "--resample) mixed in themselves, not as Gaussian noise - every one at every level of --snrs")
    c.add_argument('--augment-maskers', action='store', type=augment_maskers_argument, dest='augment_maskers', default=argparse.SUPPRESS,
                   help="train --engine hip --from-wav --augment-masker-snrs: comma-separated recordings, as noisesweep's --maskers; "
                        "every epoch each file is rendered under a segment of one of them at one of the SNRs, or without")
    c.add_argument('--augment-masker-snrs', action='store', type=augment_masker_snrs_argument, dest='augment_masker_snrs',
                   default=argparse.SUPPRESS, help="train --augment-maskers: comma-separated SNRs in dB of the maskers")
    c.add_argument('--augment-cutoffs', action='store', type=augment_cutoffs_argument, dest='augment_cutoffs', default=argparse.SUPPRESS,
                   help="train --engine hip --from-wav: comma-separated envelope cutoffs in Hz, as lpfsweep's --cutoffs; every epoch "
                        "the envelopes of each file are low-passed at one of them, or left unfiltered (not with --lpf)")
    c.add_argument('--seed', action='store', type=int, dest='seed',
                   help="noisesweep: seed of the noise (default 0); train --from-wav: seed of the weights, the order and the noise")
    c.add_argument('--save-wavs', action='store_true', dest='save_wavs',
                   help="noisesweep: also write the noisy WAV files, as evalnoise does")
    # (absent from the parsed arguments unless given: the commands parse as before without them)
    c.add_argument('--by', action='store', dest='by', choices=('set', 'region', 'speaker', 'phoneme'), default=argparse.SUPPRESS,
                   help="test: break the result down by this column of the label CSV")
    c.add_argument('--rows', action='store', dest='rows', choices=('test', 'train', 'all'), default=argparse.SUPPRESS,
                   help="test: score the TEST rows of the label CSV (default), the others, or all of them")
    # (absent from the parsed arguments unless given: the commands parse as before without it)
    c.add_argument('--accuracy', nargs='?', choices=('reference', 'centre'), const='reference', default=argparse.SUPPRESS,
                   dest='accuracy',
                   help="eval / evalnoise / evalrand / noisesweep: accuracy against the labels of the file's .FB / .PHN; "
                        "'reference' (the bare flag) compares the row index with the label timepoint as the reference does, "
                        "'centre' the row's centre sample")
    c.add_argument('--resample', action='store_true', default=argparse.SUPPRESS, dest='resample',
                   help="eval / evalnoise / evalrand / noisesweep: bring every file to FRAMERATE of configF2CNN.conf and to one "
                        "channel on the device first (any rate; 8 / 16 / 24 / 32-bit and float RIFF files; stereo is averaged)")
    c.add_argument('--figure', action='store_true', default=argparse.SUPPRESS, dest='figure',
                   help="eval / evalnoise / evalrand: also write graphs/FallingOrRising/<basename>.png, the decisions over the "
                        "gammatonegram and the probability of 'rising' over time")
    c.add_argument('--figure-width', action='store', type=int, default=argparse.SUPPRESS, dest='figure_width',
                   help="--figure: columns of the picture (default 1600)")
    c.add_argument('--occlusion', nargs='?', type=band_and_stride, const=(8, 8), default=argparse.SUPPRESS, dest='occlusion',
                   metavar='BAND[:STRIDE]',
                   help="eval / evalnoise / evalrand: the occlusion map - every window evaluated again with each band of BAND "
                        "channels (one every STRIDE channels; the bare flag: 8:8, BAND alone: STRIDE = BAND) blanked; a table per "
                        "patch, occlusion_* keys in the .npz and graphs/Occlusion/<basename>.png, --figure-width columns wide")
    c.add_argument('--occlusion-rows', type=band_and_stride, default=argparse.SUPPRESS, dest='occlusion_rows',
                   metavar='RBAND[:RSTRIDE]', help="--occlusion: blank bands of RBAND window rows as well (no picture then)")
    c.add_argument('--occlusion-fill', type=float, default=argparse.SUPPRESS, dest='occlusion_fill', metavar='V',
                   help="--occlusion: the value a blanked cell takes, in [0, 1] (default 0, a normalised window's minimum)")
    c.add_argument('--saliency', action='store_true', default=argparse.SUPPRESS, dest='saliency',
                   help="eval / evalnoise / evalrand: the saliency map - the gradient of P(rising) at every cell of every window, one "
                        "backward pass on the device; a table per band of channels, saliency_* keys in the .npz and "
                        "graphs/Saliency/<basename>.png, --figure-width columns wide; not together with --occlusion")
    c.add_argument('--segments', action='store_true', default=argparse.SUPPRESS, dest='segments',
                   help="eval / evalnoise / evalrand: the decisions smoothed into transitions by a two-state decoder on the device; a "
                        "table of runs, with the file's .PHN a table per phoneme, and segments_* keys in the .npz")
    c.add_argument('--dwell', type=float, default=argparse.SUPPRESS, dest='dwell', metavar='MS',
                   help="--segments: the expected time in a state, in ms (default three label frames, 30 ms at 16 kHz; a default, not a "
                        "tuned value)")
    c.add_argument('--segments-weight', type=segments_weight, default=argparse.SUPPRESS, dest='segments_weight', metavar='auto|X',
                   help="--segments: the weight of a row's log-odds (default auto: min(1, hop / STEP), a heuristic for overlapping rows)")
    c.add_argument('--saliency-bands', type=int, default=argparse.SUPPRESS, dest='saliency_bands', metavar='N',
                   help="--saliency: channels per line of the table (default 8)")
    g = sub.add_parser('plot', help='plotting commands')
    g.add_argument('plot_command', choices=PLOT)
    which = g.add_mutually_exclusive_group()
    which.add_argument('--file', '-f', dest='file', nargs='?')
    which.add_argument('--all', action='store_true', dest='all_files', help="gtg: every resources/f2cnn/*/*.WAV, sorted")
    g.add_argument('--width', action='store', type=int, dest='width', default=1600, help="gtg: columns of the picture")
    g.add_argument('--pool', action='store', dest='pool', choices=('mean', 'max'), default='mean',
                   help="gtg: how the samples of a column are reduced")
    g.add_argument('--cutoff', '-c', action='store', dest='CUTOFF', type=int,
                   help="low pass filter the envelopes with this cutoff frequency")
    g.add_argument('--formant', action='store', type=int, dest='formant', default=5,
                   help="gtg: the formant track to draw, 1..4 (anything else: all four)")
    g.add_argument('--start', action='store', type=int, dest='start', default=0, help="gtg: first sample of the picture")
    g.add_argument('--end', action='store', type=int, dest='end', help="gtg: one past its last sample")
    g.add_argument('--out', action='store', dest='out', help="gtg --file: the PNG to write")
    return parser


def band_and_stride(text):
    """'BAND' or 'BAND:STRIDE', both at least 1 -> (band, stride); BAND alone: the bands lie side by side"""
    parts = text.split(':')
    try:
        values = [int(p) for p in parts]
    except ValueError:
        values = []
    if len(values) not in (1, 2) or len(values) != len(parts) or min(values) < 1:
        raise argparse.ArgumentTypeError("expected BAND or BAND:STRIDE, whole numbers of at least 1, not {!r}".format(text))
    return values[0], values[-1]


def labelled_window_files(args):
    """cnn train / cnn test: (input .npy, label .csv) as given or at their default places (f2cnn.py:126-143), or None after
    saying which of the two has still to be made"""
    import os
    inputFile = args.inputFile or args.file or os.path.join('trainingData', 'last_input_data.npy')
    labelFile = args.labelFile or os.path.join('trainingData', 'label_data.csv')
    if not os.path.isfile(inputFile):
        print("Please first generate the input data file with 'prepare input', or give one with --input")
        return None
    if not os.path.isfile(labelFile):
        print("Please first generate a label data file with 'prepare label', or give one with --label")
        return None
    return inputFile, labelFile


# The sweep commands: command -> (whether the options it does not take are refused before anything else of the command line -
# noisesweep reads --lpf, --model, --hop, --accuracy and --resample first -, what it says of --lpf if it does not take it, what to use
# instead of --figure / --occlusion, the options of which one has to be given, what is said when none is, the call with the keyword
# arguments main() made of the common options)
SWEEPS = {
    'noisesweep': (False, None, "use evalnoise {} for one level", ('snrs',),
                   "Please use --snrs to give the noise levels, e.g. --snrs 20,10,0,-3",
                   lambda E, a, kw: E.EvaluateNoiseSweep([a.file], a.snrs, seed=a.seed or 0, save_wavs=a.save_wavs, **kw,
                                                         **colour_keywords(a))),
    'lpfsweep': (True, "the cutoffs come from --cutoffs; the unfiltered level is always there", "use eval --lpf HZ {} for one cutoff",
                 ('cutoffs',), "Please use --cutoffs to give the envelope cutoffs in Hz, e.g. --cutoffs 5,10,20,50,100",
                 lambda E, a, kw: E.EvaluateCutoffSweep([a.file], a.cutoffs, **kw)),
    'reverbsweep': (True, None, "use eval {} on a WAV written with --save-wavs", ('t60', 'rir'),
                    "Please use --t60 to give the reverberation times in seconds, e.g. --t60 0.2,0.4,0.8, or --rir to give impulse "
                    "response files",
                    lambda E, a, kw: E.EvaluateReverbSweep([a.file], t60s=getattr(a, 't60', ()), rirs=getattr(a, 'rir', ()),
                                                           drr_db=getattr(a, 'drr', 0.0), seed=a.seed or 0, save_wavs=a.save_wavs, **kw)),
    'smearsweep': (True, None, "use eval {} for the sharp level", ('spreads', 'bands'),
                   "Please use --spreads to give the channel interaction in ERB, e.g. --spreads 0.5,1,2,4, or --bands to give numbers "
                   "of vocoder bands, e.g. --bands 32,16,8",
                   lambda E, a, kw: E.EvaluateSmearSweep([a.file], spreads=getattr(a, 'spreads', ()), bands=getattr(a, 'bands', ()), **kw)),
}


def colour_keywords(args):
    """what --colours / --noise-taps add to EvaluateNoiseSweep's call: nothing unless given, so that the call without them is the
    one it was"""
    kw = {}
    if 'colours' in args:
        kw['colours'] = args.colours
        if 'noise_taps' in args:
            kw['noise_taps'] = args.noise_taps
    if 'maskers' in args:
        kw['maskers'] = args.maskers
    return kw


def maskers_refusal(args):
    """What is wrong with --maskers on this command line, or None. Looks at the arguments alone."""
    if 'maskers' not in args:
        return None
    if args.cnn_command != 'noisesweep':
        if args.cnn_command in SWEEPS:
            return "--maskers is not supported by {} (the maskers belong to noisesweep)".format(args.cnn_command)
        return "--maskers only applies to 'cnn noisesweep'"
    if 'colours' in args or 'noise_taps' in args:
        return "--maskers and --colours each make the levels of a sweep: give one of them"
    if args.snrs is not None and len(args.maskers) * len(args.snrs) > NOISE_LEVELS_MAX:
        return "a noise sweep takes at most {} levels, not {} maskers x {} SNRs = {}".format(
            NOISE_LEVELS_MAX, len(args.maskers), len(args.snrs), len(args.maskers) * len(args.snrs))
    return None


def augment_maskers_refusal(args):
    """The same for --augment-maskers / --augment-masker-snrs, asked once from_wav_refusal has nothing to say"""
    given = [opt for attr, opt in (('augment_maskers', '--augment-maskers'), ('augment_masker_snrs', '--augment-masker-snrs')) if attr in args]
    if not given:
        return None
    if args.cnn_command != 'train':
        return "{} only applies to 'cnn train'".format(given[0])
    if getattr(args, 'engine', 'torch') != 'hip':
        return "{} needs --engine hip: only the library's own training step renders windows from the waves".format(given[0])
    if 'from_wav' not in args:
        return "{} needs --from-wav: stored windows cannot be rendered again under a masker".format(given[0])
    if 'augment_maskers' not in args:
        return "--augment-masker-snrs belongs to --augment-maskers"
    if 'augment_masker_snrs' not in args:
        return "--augment-maskers needs --augment-masker-snrs: a masker is drawn together with the SNR it is mixed in at"
    if len(args.augment_maskers) * len(args.augment_masker_snrs) > NOISE_LEVELS_MAX:
        return "training takes at most {} masker levels, not {} maskers x {} SNRs = {}".format(
            NOISE_LEVELS_MAX, len(args.augment_maskers), len(args.augment_masker_snrs), len(args.augment_maskers) * len(args.augment_masker_snrs))
    return None


def augment_cutoffs_refusal(args):
    """The same for --augment-cutoffs, asked once from_wav_refusal has nothing to say"""
    if 'augment_cutoffs' not in args:
        return None
    if args.cnn_command != 'train':
        return "--augment-cutoffs only applies to 'cnn train'"
    if getattr(args, 'engine', 'torch') != 'hip':
        return "--augment-cutoffs needs --engine hip: only the library's own training step renders windows from the waves"
    if 'from_wav' not in args:
        return "--augment-cutoffs needs --from-wav: stored windows cannot be rendered again at another envelope cutoff"
    if args.CUTOFF is not None:
        return "--augment-cutoffs and --lpf exclude each other: the cutoffs filter unfiltered envelopes, one cutoff per file"
    return None


def colours_refusal(args):
    """What is wrong with --colours / --noise-taps on this command line, or None. Looks at the arguments alone."""
    given = [opt for attr, opt in (('colours', '--colours'), ('noise_taps', '--noise-taps')) if attr in args]
    if not given:
        return None
    if args.cnn_command != 'noisesweep':
        if args.cnn_command in SWEEPS:
            return "{} is not supported by {} (the noise colours belong to noisesweep)".format(given[0], args.cnn_command)
        return "{} only applies to 'cnn noisesweep'".format(given[0])
    if 'colours' not in args:
        return "--noise-taps belongs to --colours"
    if args.snrs is not None and len(args.colours) * len(args.snrs) > NOISE_LEVELS_MAX:
        return "a noise sweep takes at most {} levels, not {} colours x {} SNRs = {}".format(
            NOISE_LEVELS_MAX, len(args.colours), len(args.snrs), len(args.colours) * len(args.snrs))
    return None


def from_wav_refusal(args):
    """What is wrong with --from-wav / --augment-snrs on this command line, or None. Looks at the arguments alone."""
    given = [opt for attr, opt in (('from_wav', '--from-wav'), ('augment_snrs', '--augment-snrs')) if attr in args]
    if not given:
        return None
    if args.cnn_command != 'train':
        return "{} only applies to 'cnn train'".format(given[0])
    if getattr(args, 'engine', 'torch') != 'hip':
        return "{} needs --engine hip: only the library's own training step renders windows from the waves".format(given[0])
    if 'from_wav' not in args:
        return "--augment-snrs needs --from-wav: stored windows cannot be rendered again under noise"
    return None


def rooms_refusal(args):
    """The same for --augment-t60 / --augment-rirs, asked once from_wav_refusal has nothing to say"""
    given = [opt for attr, opt in (('augment_t60', '--augment-t60'), ('augment_rirs', '--augment-rirs')) if attr in args]
    if not given:
        return None
    if args.cnn_command != 'train':
        return "{} only applies to 'cnn train'".format(given[0])
    if getattr(args, 'engine', 'torch') != 'hip':
        return "{} needs --engine hip: only the library's own training step renders windows from the waves".format(given[0])
    if 'from_wav' not in args:
        return "{} needs --from-wav: stored windows cannot be reverberated".format(given[0])
    return None


def augment_colours_refusal(args):
    """The same for --augment-colours / --augment-noise-taps, asked once from_wav_refusal has nothing to say"""
    given = [opt for attr, opt in (('augment_colours', '--augment-colours'), ('augment_noise_taps', '--augment-noise-taps')) if attr in args]
    if not given:
        return None
    if args.cnn_command != 'train':
        return "{} only applies to 'cnn train'".format(given[0])
    if 'augment_colours' not in args:
        return "--augment-noise-taps belongs to --augment-colours"
    if 'augment_snrs' not in args:
        return "--augment-colours needs --augment-snrs: a colour is drawn together with the SNR it is added at"
    if len(args.augment_colours) * len(args.augment_snrs) > NOISE_LEVELS_MAX:
        return "training takes at most {} noise levels, not {} colours x {} SNRs = {}".format(
            NOISE_LEVELS_MAX, len(args.augment_colours), len(args.augment_snrs), len(args.augment_colours) * len(args.augment_snrs))
    return None


def augment_smear_refusal(args):
    """The same for --augment-spreads / --augment-bands, asked once from_wav_refusal has nothing to say"""
    given = [opt for attr, opt in (('augment_spreads', '--augment-spreads'), ('augment_bands', '--augment-bands')) if attr in args]
    if not given:
        return None
    if args.cnn_command != 'train':
        return "{} only applies to 'cnn train'".format(given[0])
    if getattr(args, 'engine', 'torch') != 'hip':
        return "{} needs --engine hip: only the library's own training step renders windows from the waves".format(given[0])
    if 'from_wav' not in args:
        return "{} needs --from-wav: stored windows are normalised already and cannot be mixed across their channels".format(given[0])
    levels = len(getattr(args, 'augment_spreads', ())) + len(getattr(args, 'augment_bands', ()))
    if levels > SMEAR_LEVELS_MAX:
        return "training takes at most {} spectral resolutions, not {}".format(SMEAR_LEVELS_MAX, levels)
    return None


def segments_weight(text):
    """--segments-weight: 'auto' or a number in (0, 16]"""
    if text == 'auto':
        return text
    try:
        value = float(text)
    except ValueError:
        value = 0.0
    if not 0.0 < value <= 16.0:
        raise argparse.ArgumentTypeError("--segments-weight takes 'auto' or a number in (0, 16], not {!r}".format(text))
    return value


NO_SWEEP_SEGMENTS = "the sweeps print no transitions; the decoding entry points take their batches as they are"


def sweep_refusal(args, no_lpf, instead):
    """says which option the sweep does not take, if one was given (an option that was not given is absent, None or False)"""
    for attr, option, why in (('CUTOFF', '--lpf', no_lpf), ('figure', '--figure', instead), ('occlusion', '--occlusion', instead),
                              ('saliency', '--saliency', instead), ('segments', '--segments', NO_SWEEP_SEGMENTS)):
        if why and getattr(args, attr, None) not in (None, False):
            print("{} is not supported by {} ({})".format(option, args.cnn_command, why.format(option)))
            return True
    return False


def main(argv=None):
    args = build_parser().parse_args(argv)
    if 'prepare_command' in args:
        if args.from_wav and args.prepare_command != 'input':
            print("--from-wav only applies to 'prepare input'")
            return 1
        kwargs = {}
        if args.prepare_command in ('envelope', 'input', 'features'):      # f2cnn.py:112-114
            kwargs['LPF'] = args.CUTOFF is not None
            kwargs['CUTOFF'] = args.CUTOFF
        if args.prepare_command == 'input':
            if args.labelFile is not None:
                kwargs['labelFile'] = args.labelFile
            if args.inputFile is not None:
                kwargs['inputFile'] = args.inputFile
        if args.prepare_command in ('filter', 'envelope', 'features'):
            kwargs['skip_existing'] = args.skip_existing
            kwargs['metrics'] = args.metrics
        if args.prepare_command == 'filter':
            from .scripts.processing.GammatoneFiltering import FilterAllOrganisedFiles as fn
        elif args.prepare_command == 'envelope':
            from .scripts.processing.EnvelopeExtraction import ExtractAllEnvelopes as fn
        elif args.prepare_command == 'label':
            from .scripts.processing.LabelDataGenerator import GenerateLabelData as fn
        elif args.prepare_command == 'features':
            from .scripts.processing.EnvelopeExtraction import FilterAndExtractAll as fn
        elif args.from_wav:
            from .scripts.processing.InputGenerator import GenerateInputDataFromWav as fn
            kwargs['metrics'] = args.metrics
        else:
            from .scripts.processing.InputGenerator import GenerateInputData as fn
        report = fn(**kwargs)
        if getattr(report, "exit_status", 0):          # some files could not be processed (the others were)
            return report.exit_status
    elif 'cnn_command' in args:
        refusal = (from_wav_refusal(args) or rooms_refusal(args) or augment_colours_refusal(args) or augment_smear_refusal(args) or
                   augment_maskers_refusal(args) or augment_cutoffs_refusal(args) or colours_refusal(args) or maskers_refusal(args))
        if refusal:
            print(refusal)
            return 1
        if args.cnn_command == 'train' and 'from_wav' in args:
            import os
            from .scripts.CNN.Training import TrainFromWav
            labelFile = args.labelFile or os.path.join('trainingData', 'label_data.csv')
            if not os.path.isfile(labelFile):
                print("Please first generate a label data file with 'prepare label', or give one with --label")
                return 1
            rooms = {}                                         # (only when asked for: the call without rooms is the one it was)
            if 'augment_t60' in args or 'augment_rirs' in args:
                rooms = dict(t60s=tuple(getattr(args, 'augment_t60', ())), rirs=tuple(getattr(args, 'augment_rirs', ())),
                             drr_db=getattr(args, 'drr', 0.0))
            if 'augment_colours' in args:                      # (likewise)
                rooms['colours'] = tuple(args.augment_colours)
                if 'augment_noise_taps' in args:
                    rooms['noise_taps'] = args.augment_noise_taps
            if 'augment_spreads' in args or 'augment_bands' in args:
                rooms.update(spreads=tuple(getattr(args, 'augment_spreads', ())), bands=tuple(getattr(args, 'augment_bands', ())))
            if 'augment_maskers' in args:                      # (likewise)
                rooms.update(maskers=tuple(args.augment_maskers), masker_snrs=tuple(args.augment_masker_snrs))
            if 'augment_cutoffs' in args:                      # (likewise)
                rooms.update(cutoffs=tuple(args.augment_cutoffs))
            TrainFromWav(labelFile=labelFile, LPF=args.CUTOFF is not None, CUTOFF=args.CUTOFF, snrs=tuple(getattr(args, 'augment_snrs', ())),
                         seed=args.seed, **rooms)
            return 0
        if args.cnn_command == 'train':                        # f2cnn.py:126-143
            from .scripts.CNN.Training import TrainAndPlotLoss
            files = labelled_window_files(args)
            if files is None:
                return 1
            TrainAndPlotLoss(labelFile=files[1], inputFile=files[0], engine=getattr(args, 'engine', 'torch'))
            return 0
        if args.cnn_command == 'test':
            from .scripts.CNN.Training import TestModel
            files = labelled_window_files(args)
            if files is None:
                return 1
            TestModel(labelFile=files[1], inputFile=files[0], model=args.model or 'last_trained_model',
                      by=getattr(args, 'by', None), rows=getattr(args, 'rows', 'test'))
            return 0
        from .scripts.CNN import Evaluating
        kwargs = {}
        sweep = SWEEPS.get(args.cnn_command)
        if sweep and sweep[0] and sweep_refusal(args, *sweep[1:3]):
            return 1
        if args.CUTOFF is not None:                            # f2cnn.py:149-151
            kwargs['LPF'] = True
            kwargs['CUTOFF'] = args.CUTOFF
        if args.model is not None:
            kwargs['model'] = args.model
        if args.hop is not None:
            kwargs['hop'] = args.hop
            if args.hop == 'frame':
                from .config import F2Config
                kwargs['hop'] = F2Config().step
        if getattr(args, 'accuracy', None) is not None:
            kwargs['accuracy'] = args.accuracy
        if getattr(args, 'resample', False):
            kwargs['resample'] = True
        if sweep and not sweep[0] and sweep_refusal(args, *sweep[1:3]):
            return 1
        if getattr(args, 'figure', False):
            kwargs['figure'] = True
        if 'occlusion' in args:
            fill = getattr(args, 'occlusion_fill', 0.0)
            if not 0.0 <= fill <= 1.0:
                print("--occlusion-fill must lie in [0, 1], the range of a normalised window")
                return 1
            rows = getattr(args, 'occlusion_rows', (None, None))
            kwargs['occlusion'] = dict(band=args.occlusion[0], stride=args.occlusion[1], row_band=rows[0], row_stride=rows[1], fill=fill)
        elif 'occlusion_rows' in args or 'occlusion_fill' in args:
            print("--occlusion-rows and --occlusion-fill belong to --occlusion")
            return 1
        if 'saliency' in args:
            if 'occlusion' in args:
                print("--saliency and --occlusion each make the one map of a run: give one of them")
                return 1
            bands = getattr(args, 'saliency_bands', 8)
            if bands < 1:
                print("--saliency-bands must be at least 1 channel")
                return 1
            kwargs['saliency'] = bands
        elif 'saliency_bands' in args:
            print("--saliency-bands belongs to --saliency")
            return 1
        if getattr(args, 'figure_width', None) is not None and (kwargs.get('figure') or 'occlusion' in kwargs or 'saliency' in kwargs):
            kwargs['figure_width'] = args.figure_width          # (the one width of the figure and of a map)
        if 'segments' in args:
            if sweep:
                print("--segments is not supported by {} ({})".format(args.cnn_command, NO_SWEEP_SEGMENTS))
                return 1
            if getattr(args, 'dwell', 1.0) <= 0.0:
                print("--dwell must be a positive time in ms")
                return 1
            kwargs['segments'] = dict(dwell_ms=getattr(args, 'dwell', None), weight=getattr(args, 'segments_weight', 'auto'))
        elif 'dwell' in args or 'segments_weight' in args:
            print("--dwell and --segments-weight belong to --segments")
            return 1
        if args.cnn_command == 'evalrand':                     # needs no --file (unreachable in the reference CLI)
            if args.count is not None:
                kwargs['count'] = args.count
            Evaluating.EvaluateRandom(**kwargs)
            return 0
        if args.file is None:
            print("Please use --file or -f to give input file")
            return 1
        if sweep:
            if all(getattr(args, name, None) is None for name in sweep[3]):
                print(sweep[4])
                return 1
            sweep[5](Evaluating, args, kwargs)
            return 0
        kwargs['file'] = args.file
        if args.cnn_command == 'evalnoise':
            if args.SNRdB is not None:
                kwargs['SNRdB'] = args.SNRdB
            Evaluating.EvaluateWithNoise(**kwargs)
        else:
            Evaluating.EvaluateOneWavFile(**kwargs)
    elif 'plot_command' in args:
        from .scripts.plotting import PlottingProcessing
        kwargs = dict(start=args.start, end=args.end, formantToPlot=args.formant, width=args.width, pool=args.pool,
                      LPF=args.CUTOFF is not None, CUTOFF=args.CUTOFF)
        if args.all_files:
            import glob
            import os
            files = sorted(glob.glob(os.path.join('resources', 'f2cnn', '*', '*.WAV')))
            if not files:
                print("NO FILES FOUND, PLEASE ORGANIZE FILES")
                return 1
        elif args.file is None:
            print("Please use --file or -f to give input file, or --all")
            return 1
        else:
            files = [args.file]
            kwargs['out'] = args.out
        report = PlottingProcessing.PlotGammatonegrams(files, **kwargs)
        if report.exit_status:
            return report.exit_status
    elif args.configure:
        from .config import write_default
        print("Saving configuration file as '{}'".format(write_default()))
    else:
        print("No valid command given.")
        print("For help, use python -m f2cnn_amd --help")
        return 1
    return 0
