"""Float64 references for bus convolvers whose IR may have one, two or four channels (the rules of include/gas_amd.h).
A four-channel ("true stereo") IR is [LL, LR, RL, RR]: channel c = 2 i + e goes from input ear i to output ear e and

    y_e[t] = dry * x_e[t] + wet * sum_{j < T} ( h_{0e}[j] * x_0[t - j] + h_{1e}[j] * x_1[t - j] ),   x[t] = 0 for t < 0

TrueStereoRef is that rule as written, a direct-form sum over a kept history with ConvRef's interface; one- and
two-channel IRs are the diagonal case.  TrueStereoFadeRef is conv_fade_ref's state machine over such states.
TrueStereoPartitionModel restates the device bookkeeping (one ring per input ear, four sets of IR spectra).
whole_signal is the FFT of the whole input, for runs too long for the direct form; the CPU tests pin it to the direct form."""
import numpy as np

from conv_fade_ref import ConvFadeRef
from conv_ref import N_FFT, PartitionModel


def matrix(ir):
    """[channels][taps] (or [taps]), channels 1, 2 or 4 -> h[i][e][taps] float64, input ear i to output ear e."""
    h = np.atleast_2d(np.asarray(ir, dtype=np.float64))
    assert h.ndim == 2 and h.shape[0] in (1, 2, 4) and h.shape[1] >= 1
    if h.shape[0] == 4:
        return h.reshape(2, 2, -1).copy()
    m = np.zeros((2, 2, h.shape[1]))
    m[0, 0], m[1, 1] = h[0], h[-1]  # no cross-feed; a one-channel IR serves both ears
    return m


class TrueStereoRef:
    def __init__(self, ir, dry=0.0, wet=1.0):
        self.h = matrix(ir)
        self.dry, self.wet = float(dry), float(wet)
        self.x = np.zeros((0, 2))  # every frame since the last reset

    def set_ir(self, ir):
        self.h = matrix(ir)  # the history stays

    def set_levels(self, dry, wet):
        self.dry, self.wet = float(dry), float(wet)

    def reset(self):
        self.x = np.zeros((0, 2))

    def process(self, block):
        """block [F][2] -> [F][2] float64."""
        b = np.asarray(block, dtype=np.float64)
        t0 = self.x.shape[0]
        self.x = np.concatenate([self.x, b])
        T = self.h.shape[2]
        # past[i]: rows x_i[t - T + 1 .. t] for every t of this block, zeros before the first frame
        past = [np.lib.stride_tricks.sliding_window_view(np.concatenate([np.zeros(T - 1), self.x[:, i]])[t0 : t0 + b.shape[0] + T - 1], T) for i in range(2)]
        out = np.empty_like(b)
        for e in range(2):
            direct, cross = past[e] @ self.h[e, e, ::-1], past[1 - e] @ self.h[1 - e, e, ::-1]
            out[:, e] = self.dry * b[:, e] + self.wet * (direct + cross)
        return out


class TrueStereoFadeRef(ConvFadeRef):
    """ConvFadeRef whose states A and B are TrueStereoRefs: any mix of one-, two- and four-channel IRs."""

    def __init__(self, frames, ir, dry=0.0, wet=1.0):
        super().__init__(frames, [1.0], dry, wet)
        self.a, self.ir_a = TrueStereoRef(ir, dry, wet), ir

    def fade_to(self, ir, dry, wet, fade_blocks):
        if fade_blocks == 0 or self.b is not None:  # a hard switch, or a pending target: the base class builds no state
            return super().fade_to(ir, dry, wet, fade_blocks)
        super().fade_to([1.0], dry, wet, fade_blocks)
        self.b, self.ir_b = TrueStereoRef(ir, dry, wet), ir


class TrueStereoPartitionModel(PartitionModel):
    """PartitionModel with H[i][e][k][513]: output ear e sums both input ears' rings, partition by partition."""

    def set_ir(self, ir):
        h = matrix(ir)
        F = self.F
        self.k_ir = -(-h.shape[2] // F)
        assert self.k_ir <= self.K
        pad = np.zeros((2, 2, self.k_ir * F))
        pad[:, :, : h.shape[2]] = h
        win = np.zeros((2, 2, self.k_ir, N_FFT))
        win[..., :F] = pad.reshape(2, 2, self.k_ir, F)
        self.H = np.fft.rfft(win, axis=3)

    def process(self, block):
        F, K = self.F, self.K
        b = np.asarray(block, dtype=np.float64)
        self.pos = (self.pos + 1) % K
        for i in range(2):  # one new spectrum per input ear
            w = np.zeros(N_FFT)
            w[N_FFT - 2 * F : N_FFT - F] = self.prev[:, i]
            w[N_FFT - F :] = b[:, i]
            self.ring[i, self.pos] = np.fft.rfft(w)
        out = np.empty_like(b)
        for e in range(2):
            Y = np.zeros(N_FFT // 2 + 1, dtype=np.complex128)
            for k in range(self.k_ir):
                r = (self.pos + K - k) % K
                Y += self.ring[e, r] * self.H[e, e, k] + self.ring[1 - e, r] * self.H[1 - e, e, k]
            out[:, e] = self.dry * b[:, e] + self.wet * np.fft.irfft(Y, N_FFT)[N_FFT - F :]
        self.prev = b.copy()
        return out


def whole_signal(ir, x, dry=0.0, wet=1.0):
    """The rule over a whole input x [frames][2] from a fresh instance, by one float64 FFT -> [frames][2]."""
    h = matrix(ir)
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0] + h.shape[2] - 1
    X = np.fft.rfft(x, n, axis=0)
    out = np.empty_like(x)
    for e in range(2):
        Y = X[:, 0] * np.fft.rfft(h[0, e], n) + X[:, 1] * np.fft.rfft(h[1, e], n)
        out[:, e] = dry * x[:, e] + wet * np.fft.irfft(Y, n)[: x.shape[0]]
    return out
