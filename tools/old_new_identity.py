"""Outputs of two builds of the library compared bit for bit (diagnostic; profiles/r08_a_old_new_identity.txt).
    python tools/old_new_identity.py run LIB OUT.json     digests of every case's outputs with that library
    python tools/old_new_identity.py compare OLD.json NEW.json    the table "case: identical / differs"
Cases: f2_filterbank_envelope_fused, f2_eval_batch, f2_eval_utterance (one utterance) and f2_input_batch on single utterances of
1 700, 1 761, 16 000, 40 000 and 70 000 samples and on the 34-length ragged batch of tests/test_gpu_spectral.py; LPF off and
50 Hz; int16 waves, host memory, 128 channels."""
import hashlib, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

C, RADIUS, STEP = 128, 5, 160
R = 2 * RADIUS + 1
RAGGED = [16000, 15999, 9000, 8193, 16320, 16321, 4097, 5000, 8128, 8129, 300, 16384, 20000, 1, 32704, 32705, 16385,
          27001, 40000, 32769, 65472, 65473, 50001, 65536, 33333, 70000, 16128, 16129, 7936, 7937, 32512, 32513, 65280, 65281]
BATCHES = [(f"one utterance of {n}", [n]) for n in (1700, 1761, 16000, 40000, 70000)] + [("ragged batch of 34", RAGGED)]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def run(lib, out):
    from f2cnn_amd import build
    build.LIB_PATH = os.path.abspath(lib)
    import f2cnn_oracle as orc
    from f2cnn_amd import _lib
    from f2cnn_amd.model import F2CNNModel
    ctx = _lib.Context(0)
    coefs = orc.make_erb_filters(16000, orc.centre_freqs(16000, C, 100))
    h = F2CNNModel.glorot(11).handle(ctx)
    res = {}
    for name, lens in BATCHES:
        waves = [orc.synth_utterance(500 + i, n) for i, n in enumerate(lens)]
        flat = np.concatenate(waves)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        B, total = len(lens), int(offs[-1])
        nbs = [max(n - R * STEP, 0) for n in lens]
        # two centres per utterance that has room for a window: the first and the last legal one
        cs = [np.array([RADIUS * STEP, n - 1 - RADIUS * STEP], np.int64) if n > 2 * RADIUS * STEP else np.zeros(0, np.int64) for n in lens]
        coffs = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
        for lpf in (False, True):
            cut = 50.0 if lpf else 0.0
            tag = f"{name}, {'LPF 50 Hz' if lpf else 'no LPF'}"
            env = np.zeros((C * total,))
            ctx.filterbank_envelope_fused(flat, _lib.WAVE_I16, offs, coefs, B, C, lpf, cut, _lib.FFT_F32, env, None, _lib.MEM_HOST)
            res[f"f2_filterbank_envelope_fused: {tag}"] = digest(env)
            sc, lb = np.zeros((sum(nbs), 2), np.float32), np.zeros(sum(nbs), np.uint8)
            ctx.eval_batch(h, flat, _lib.WAVE_I16, offs, coefs, B, C, lpf, cut, _lib.FFT_F32, RADIUS, STEP, sc, lb, _lib.MEM_HOST)
            res[f"f2_eval_batch: {tag}"] = digest(sc, lb)
            if B == 1:
                sc, lb, env = np.zeros((nbs[0], 2), np.float32), np.zeros(nbs[0], np.uint8), np.zeros((C, total))
                nb = ctx.eval_utterance(h, flat, _lib.WAVE_I16, total, coefs, C, lpf, cut, _lib.FFT_F32, RADIUS, STEP, env, sc, lb,
                                        _lib.MEM_HOST)
                res[f"f2_eval_utterance: {tag}"] = digest(sc, lb, env, np.int64(nb))
            win = np.zeros((int(coffs[-1]), R, C), np.float32)
            ctx.input_batch(flat, _lib.WAVE_I16, offs, coefs, B, C, lpf, cut, _lib.FFT_F32, coffs,
                            np.concatenate(cs) if len(cs) else np.zeros(0, np.int64), RADIUS, STEP, True, win, _lib.MEM_HOST)
            res[f"f2_input_batch: {tag}"] = digest(win)
            print(tag, "done", flush=True)
    ctx.close()
    json.dump(res, open(out, "w"), indent=1)


def compare(a, b):
    old, new = json.load(open(a)), json.load(open(b))
    assert list(old) == list(new)
    bad = 0
    for k in old:
        same = old[k] == new[k]
        bad += not same
        print(f"{k}: {'identical' if same else 'DIFFERS'} ({old[k]}{'' if same else ' / ' + new[k]})")
    print(f"{len(old) - bad} of {len(old)} cases identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(run(*sys.argv[2:4]) if sys.argv[1] == "run" else compare(*sys.argv[2:4]))
