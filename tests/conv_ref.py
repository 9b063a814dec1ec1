"""Float64 references for the bus convolvers (gas_conv_*; the rule of include/gas_amd.h):

    y_e[t] = dry * x_e[t] + wet * sum_{j < T} h_e[j] * x_e[t - j],   x[t] = 0 for t < 0

ConvRef is the rule as written: a direct-form sum over a kept input history, nothing of the kernels' structure.
PartitionModel restates the kernels' bookkeeping -- uniform partitions of F taps, a ring of K input spectra, 1024-point
windows [zeros, previous block, this block] whose last F outputs are kept -- in float64 with numpy's FFT, so the
indexing can be checked against ConvRef without a GPU."""
import numpy as np

N_FFT = 1024


def ears(ir):
    """[channels][taps] (or [taps]) -> [2][taps] float64: a one-channel IR serves both ears."""
    h = np.atleast_2d(np.asarray(ir, dtype=np.float64))
    assert h.ndim == 2 and h.shape[0] in (1, 2) and h.shape[1] >= 1
    return np.stack([h[0], h[-1]])


class ConvRef:
    def __init__(self, ir, dry=0.0, wet=1.0):
        self.h = ears(ir)
        self.dry, self.wet = float(dry), float(wet)
        self.x = np.zeros((0, 2))  # every frame since the last reset

    def set_ir(self, ir):
        self.h = ears(ir)  # the history stays: it does not depend on the IR

    def set_levels(self, dry, wet):
        self.dry, self.wet = float(dry), float(wet)

    def reset(self):
        self.x = np.zeros((0, 2))

    def process(self, block):
        """block [F][2] -> [F][2] float64."""
        b = np.asarray(block, dtype=np.float64)
        t0 = self.x.shape[0]
        self.x = np.concatenate([self.x, b])
        out = np.empty_like(b)
        T = self.h.shape[1]
        for e in range(2):
            # rows of `past`: x[t - T + 1 .. t] for every t of this block, zeros before the first frame
            x = np.concatenate([np.zeros(T - 1), self.x[:, e]])[t0 : t0 + b.shape[0] + T - 1]
            past = np.lib.stride_tricks.sliding_window_view(x, T)
            out[:, e] = self.dry * b[:, e] + self.wet * (past @ self.h[e, ::-1])
        return out


class PartitionModel:
    """One instance as the device keeps it: ring[e][K][513] input spectra, the previous block, a ring position."""

    def __init__(self, frames, max_ir_taps, ir, dry=0.0, wet=1.0):
        self.F = int(frames)
        assert 2 * self.F <= N_FFT
        self.K = -(-int(max_ir_taps) // self.F)
        self.dry, self.wet = float(dry), float(wet)
        self.set_ir(ir)
        self.reset()

    def set_ir(self, ir):
        h = ears(ir)
        F = self.F
        self.k_ir = -(-h.shape[1] // F)
        assert self.k_ir <= self.K
        pad = np.zeros((2, self.k_ir * F))
        pad[:, : h.shape[1]] = h
        win = np.zeros((2, self.k_ir, N_FFT))
        win[:, :, :F] = pad.reshape(2, self.k_ir, F)  # partition k at the front of its window, zeros behind
        self.H = np.fft.rfft(win, axis=2)

    def set_levels(self, dry, wet):
        self.dry, self.wet = float(dry), float(wet)

    def reset(self):
        self.ring = np.zeros((2, self.K, N_FFT // 2 + 1), dtype=np.complex128)
        self.prev = np.zeros((self.F, 2))
        self.pos = self.K - 1  # the position of the newest spectrum; the first block goes to 0

    def process(self, block):
        F, K = self.F, self.K
        b = np.asarray(block, dtype=np.float64)
        self.pos = (self.pos + 1) % K
        out = np.empty_like(b)
        for e in range(2):
            w = np.zeros(N_FFT)
            w[N_FFT - 2 * F : N_FFT - F] = self.prev[:, e]
            w[N_FFT - F :] = b[:, e]
            self.ring[e, self.pos] = np.fft.rfft(w)
            Y = np.zeros(N_FFT // 2 + 1, dtype=np.complex128)
            for k in range(self.k_ir):  # only the partitions the IR has
                Y += self.ring[e, (self.pos + K - k) % K] * self.H[e, k]
            y = np.fft.irfft(Y, N_FFT)[N_FFT - F :]
            out[:, e] = self.dry * b[:, e] + self.wet * y
        self.prev = b.copy()
        return out


def run_blocks(model, blocks):
    return np.stack([model.process(b) for b in blocks])
