"""Numerical prototype of the spectral path with the row padded IN FRONT (kernel KS).

proto_spectral.py forms  Y(k) = H_c X(k) + w_k^N u^4 Q(w_k) / gain  for the row padded BEHIND sample N: the factor w_k^N (`zeta`
there) moves the ringing term to the cut between row and padding. With the utterance at the indices [M - N, M) of the transform
the cut falls on index M = 0, w_k^M = 1:

    Y'(k) = conj(w_k^N) Y(k) = H_c X'(k) + u^4 Q(w_k) / gain,     X' = DFT_M(x padded in front)

The filter's state at the row's end, hence the digits of Q, is the same (zeros fed to a zero state leave it zero), and the analytic
signal of a circularly shifted sequence is the shifted analytic signal: the envelope is read M - N indices later.

Run:  python tests/diag/proto_front_padding.py   (CPU only; float32 emulation of the device arithmetic)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, '.')
import proto_spectral as ps   # noqa: E402
from proto_spectral import orc, F32, C64   # noqa: E402


def spectral_envelope_front(x, coefs, f32=True, tail_tol=1e-10, fft32=True, return_pad=False):
    """Envelope rows (C, N) from the front-padded formulation; with return_pad also max |Re a| over the padding [0, M - N)
    relative to the row maximum, per channel (the accuracy guard's quantity)."""
    N = len(x)
    M = orc.padded_length(N)
    H = M // 2
    npad = M - N
    xp = np.zeros(M)
    xp[npad:] = x
    X = np.fft.rfft(xp)                    # float64 forward transform of the front-padded utterance
    w, Ht, ut = ps.tables(coefs, M)
    cplx = C64 if f32 else np.complex128
    real = F32 if f32 else np.float64
    Xc, wc = X.astype(cplx), w.astype(cplx)
    env = np.zeros((len(coefs), N))
    pad = np.zeros(len(coefs))
    for c, row in enumerate(coefs):
        Ns, D, gain = ps.section_polys(row)
        last = ps.run_sections_tail(x, row, ps.tail_len(row, tail_tol))
        dg = ps.dadic_digits(row, last)
        rho = [(real(d[0] / gain), real(d[1] / gain)) for d in dg]
        Hc, uc = Ht[c].astype(cplx), ut[c].astype(cplx)

        def rj(j):
            return (rho[j][0] + rho[j][1] * wc).astype(cplx)
        t = rj(0)
        for j in (1, 2, 3):
            t = (rj(j) + uc * t).astype(cplx)
        Y = (Xc * Hc + (uc * t).astype(cplx)).astype(cplx)      # no phase factor on the ringing term
        A = 2 * Y
        A[0] = Y[0]
        A[H] = Y[H]
        Ae = A[:H].copy()
        Ao = (A[:H] * np.conj(wc[:H])).astype(cplx)
        Ae[0] = A[0] + A[H]
        Ao[0] = A[0] - A[H]
        if f32 and fft32:
            import scipy.fft as sfft
            ae, ao = sfft.ifft(Ae.astype(C64)), sfft.ifft(Ao.astype(C64))
        else:
            ae, ao = np.fft.ifft(Ae.astype(np.complex128)), np.fft.ifft(Ao.astype(np.complex128))
        a = np.empty(M, dtype=np.complex128)
        a[0::2] = ae / 2
        a[1::2] = ao / 2
        env[c] = np.abs(a[npad:])
        pad[c] = np.abs(a[:npad].real).max() / env[c].max() if npad else 0.0
    return (env, pad) if return_pad else env


def compare(x, coefs):
    """(front against the oracle, back against the oracle, front against back, padding residual): worst channel each"""
    ref = np.abs(np.array([orc.padded_hilbert(r) for r in orc.erb_filterbank(x, coefs)]))
    front, pad = spectral_envelope_front(x, coefs, return_pad=True)
    back = ps.spectral_envelope(x, coefs)
    return ps.relerr(front, ref).max(), ps.relerr(back, ref).max(), ps.relerr(front, back).max(), pad.max()


def main():
    fs = 16000
    rng = np.random.default_rng(2027)
    coefs = orc.make_erb_filters(fs, orc.centre_freqs(fs, 128, 100))[[0, 9, 40, 90, 127]]
    cases = {f'noise{n}': np.clip(np.round(rng.standard_normal(n) * 3000), -32768, 32767) for n in (16000, 15999, 9000, 4097, 16128)}
    t = np.arange(16000) / fs
    cases['lowsine+hiss'] = np.round(20000 * np.sin(2 * np.pi * 120 * t) + 3 * rng.standard_normal(16000))
    imp = np.zeros(16000)
    imp[15990] = 32767
    cases['impulse_end'] = imp
    for name, x in cases.items():
        f, b, fb, pad = compare(x, coefs)
        print(f'{name:14s} front {f:.2e}  back {b:.2e}  front against back {fb:.2e}  padding residual {pad:.2e}')


if __name__ == '__main__':
    main()
