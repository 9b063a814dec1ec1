"""Float64 references for gas_conv_fade_to (the fade rule of include/gas_amd.h), on top of conv_ref:

    y[t] = (1 - s) * y^A[t] + s * y^B[t],   s = (float)(b * F + i) * (1.0f / (float)(N * F))   in float32

for frame i of the b-th of the N calls of a fade from state A = (ir, dry, wet) to state B, y^S the rule of conv_ref
evaluated with state S over the instance's one input history.

ConvFadeRef is the rule as written: two direct-form states (conv_ref.ConvRef) over one history, a pending target, and
set_ir / set_levels / reset ending a fade as the header says.  DualPartitionModel restates the device bookkeeping: one
ring of input spectra, two sets of IR spectra multiplied over it, two back transforms and a lerp."""
import numpy as np

from conv_ref import N_FFT, ConvRef, PartitionModel, ears

MAX_FADE_BLOCKS = 4096


def fade_s(frames, fade_blocks, b):
    """s of the F frames of call b of a fade over fade_blocks calls: float32 arithmetic, returned as float64."""
    t = (np.arange(frames, dtype=np.int64) + b * frames).astype(np.float32)
    s = t * (np.float32(1.0) / np.float32(fade_blocks * frames))
    assert s.dtype == np.float32
    return s.astype(np.float64)


class ConvFadeRef:
    """IRs are named by their arrays: a target is (ir, dry, wet)."""

    def __init__(self, frames, ir, dry=0.0, wet=1.0):
        self.F = int(frames)
        self.a = ConvRef(ir, dry, wet)  # state A, and the history
        self.ir_a = ir
        self.b = None  # state B while a fade is in progress: a ConvRef that is handed A's history before every call
        self.ir_b = None
        self.n = self.pos = 0
        self.pending = None  # (ir, dry, wet, fade_blocks)

    # -- the state machine
    def _land(self):
        x = self.a.x
        self.a, self.ir_a = self.b, self.ir_b
        self.a.x = x
        self.b = self.ir_b = None
        self.n = self.pos = 0

    def _end(self):
        if self.b is not None:
            self._land()
        self.pending = None

    def fade_to(self, ir, dry, wet, fade_blocks):
        assert 0 <= fade_blocks <= MAX_FADE_BLOCKS and np.isfinite(dry) and np.isfinite(wet)
        if fade_blocks == 0:
            self.set_ir(ir)
            self.set_levels(dry, wet)
        elif self.b is not None:
            self.pending = (ir, dry, wet, fade_blocks)  # the latest wins
        else:
            self.b, self.ir_b = ConvRef(ir, dry, wet), ir
            self.n, self.pos = int(fade_blocks), 0

    def fade_remaining(self):
        return self.n - self.pos + (self.pending[3] if self.pending else 0)

    def set_ir(self, ir):
        self._end()
        self.a.set_ir(ir)
        self.ir_a = ir

    def set_levels(self, dry, wet):
        self._end()
        self.a.set_levels(dry, wet)

    def reset(self):
        if self.b is not None:
            self._land()
            if self.pending:
                ir, dry, wet, _ = self.pending
                self.a.set_ir(ir)
                self.a.set_levels(dry, wet)
                self.ir_a = ir
        self.pending = None
        self.a.reset()

    def named(self):
        """The IR arrays the instance names: A's, B's, a pending target's."""
        return [h for h in (self.ir_a, self.ir_b, self.pending[0] if self.pending else None) if h is not None]

    # -- a call that names the instance
    def process(self, block):
        if self.b is None:
            return self.a.process(block)
        self.b.x = self.a.x  # one history
        ya, yb = self.a.process(block), self.b.process(block)
        s = fade_s(self.F, self.n, self.pos)[:, None]
        self.pos += 1
        if self.pos == self.n:
            self._land()
            if self.pending:
                ir, dry, wet, n = self.pending
                self.pending = None
                self.fade_to(ir, dry, wet, n)
        return (1.0 - s) * ya + s * yb


class DualPartitionModel(PartitionModel):
    """PartitionModel with a fade: state B's spectra HB next to H over the one ring, ring position and previous block."""

    def __init__(self, frames, max_ir_taps, ir, dry=0.0, wet=1.0):
        super().__init__(frames, max_ir_taps, ir, dry, wet)
        self.n = self.fade_pos = 0

    def fade_to(self, ir, dry, wet, fade_blocks):
        assert self.n == 0 and fade_blocks >= 1
        a = (self.H, self.k_ir)
        self.set_ir(ir)  # partitions of B's own length
        self.HB, self.k_irB = self.H, self.k_ir
        self.H, self.k_ir = a
        self.dryB, self.wetB = float(dry), float(wet)
        self.n, self.fade_pos = int(fade_blocks), 0

    def _back(self, e, H, k_ir):
        Y = np.zeros(N_FFT // 2 + 1, dtype=np.complex128)
        for k in range(k_ir):
            Y += self.ring[e, (self.pos + self.K - k) % self.K] * H[e, k]
        return np.fft.irfft(Y, N_FFT)[N_FFT - self.F :]

    def process(self, block):
        if self.n == 0:
            return super().process(block)
        F = self.F
        b = np.asarray(block, dtype=np.float64)
        self.pos = (self.pos + 1) % self.K
        s = fade_s(F, self.n, self.fade_pos)
        out = np.empty_like(b)
        for e in range(2):
            w = np.zeros(N_FFT)
            w[N_FFT - 2 * F : N_FFT - F] = self.prev[:, e]
            w[N_FFT - F :] = b[:, e]
            self.ring[e, self.pos] = np.fft.rfft(w)  # one spectrum per block and ear, whatever the fade
            ya = self.dry * b[:, e] + self.wet * self._back(e, self.H, self.k_ir)
            yb = self.dryB * b[:, e] + self.wetB * self._back(e, self.HB, self.k_irB)
            out[:, e] = (1.0 - s) * ya + s * yb
        self.prev = b.copy()
        self.fade_pos += 1
        if self.fade_pos == self.n:
            self.H, self.k_ir, self.dry, self.wet = self.HB, self.k_irB, self.dryB, self.wetB
            self.n = self.fade_pos = 0
        return out


__all__ = ["ConvFadeRef", "DualPartitionModel", "fade_s", "ears", "MAX_FADE_BLOCKS"]
