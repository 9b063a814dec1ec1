"""The source window of _mix_from_playback_list (audio_spatializer.cpp:367-408) over a whole resident stream, written
down once in numpy: what csrc/k_sample_sources.hip's header states, and what the fused prologues (load_window<true>
in csrc/gas_hrtf_wave.h) and the host's cursor mirror (gas_process_block_streams) must agree with.

    row[i] = S[pos - 64 + i]   (zero for frames before the playback's start: the zeroed initial lookahead)
    mixed  = min(F, len - pos) fresh frames; pos += mixed
    mixed != F: row[mixed + k] *= env[k] for k < 64, row[mixed + 64 ..] = 0, has_frames clears; afterwards zeros

Every value is a float32 and every operation is rounded on its own (the sampler is compiled with fp contract off), so a
row is comparable bit for bit.  Nothing loops here: compose with stream_loop_ref.unroll for that."""
import numpy as np

LOOKAHEAD = 64
FORMATS = ["s16_mono", "s16_stereo", "f32_mono", "f32_stereo"]
F32 = np.float32
PITCHES = [0.125, 0.5, 0.97, 1.0, 1.06, 2.0, 8.0]  # 0.125 and 8 are the ends of the doppler clamp


def moving_pitch(cb):
    """A pitch that changes every block, the ends of the clamp included."""
    return (PITCHES + [0.7, 1.9])[(5 * cb + 3) % 9]


def fade_table():
    """env[k] = 0.96^(k+1) * (64 - k) / 64 by the reference's running f32 product and f32 divide (:382-392)."""
    env = np.zeros(LOOKAHEAD, F32)
    decay = F32(1.0)
    for k in range(LOOKAHEAD):
        decay = F32(decay * F32(0.96))
        env[k] = F32(F32(decay * F32(F32(LOOKAHEAD) - F32(k))) / F32(LOOKAHEAD))
    return env


ENV = fade_table()


def make_pcm(rng, frames, fmt):
    shape = (frames,) if fmt.endswith("mono") else (frames, 2)
    x = rng.uniform(-0.5, 0.5, shape)
    return (x * 32767).astype(np.int16) if fmt.startswith("s16") else x.astype(np.float32)


def to_float_stereo(pcm):
    """The frames the sampler hands on: int16 / 32768 (exact in f32), mono feeding both ears."""
    pcm = np.asarray(pcm)
    f = pcm.astype(F32) / F32(32768.0) if pcm.dtype == np.int16 else pcm.astype(F32, copy=False)
    return np.ascontiguousarray(np.stack([f, f], axis=1) if pcm.ndim == 1 else f)


def increment(pitch, mix_rate=48000.0):
    """[ENGINE] mix_increment as the context computes it: the f32 product mix_rate * pitch, divided and scaled in
    double, truncated."""
    return int((float(F32(mix_rate) * F32(pitch)) / float(F32(mix_rate))) * 65536.0)


def cubic_frames(S, start, off):
    """cubic_frame of k_sample_sources.hip for an int64 array of 16.16 positions: taps q-3 .. q, zero outside
    [start, len), the h01 / h10 / h11 weights and the sum operation for operation in f32."""
    off = np.asarray(off, np.int64)
    q = off >> 16
    mu = ((off & 0xFFFF).astype(F32) / F32(65536.0))[:, None]
    y = []
    for k in range(4):
        j = q - 3 + k
        ok = (j >= start) & (j < len(S))
        y.append(np.where(ok[:, None], S[np.clip(j, 0, max(len(S) - 1, 0))] if len(S) else F32(0), F32(0)).astype(F32))
    mu2 = mu * mu
    h11 = mu2 * (mu - F32(1))
    z = mu2 - h11
    h01 = z - h11
    h10 = mu - z
    return y[1] + (y[2] - y[1]) * h01 + ((y[2] - y[0]) * h10 + (y[3] - y[1]) * h11) * F32(0.5)


class Playback:
    """One playback bound with gas_source_bind_stream(start_frame): start = min(start_frame, frames)."""

    def __init__(self, pcm, start=0, resampled=False, mix_rate=48000.0):
        self.S = to_float_stereo(pcm)
        self.len = len(self.S)
        self.start = min(int(start), self.len)
        self.pos = self.start
        self.has_frames = True
        self.resampled = resampled
        self.mix_rate = mix_rate
        self.fp_pos = self.start << 16
        self.prev = None  # (fp_pos, inc) of the previous call: its last 64 outputs are this call's lookahead

    @property
    def position(self):
        """gas_stream_positions: the stream frame taken next."""
        return self.fp_pos >> 16 if self.resampled else self.pos

    def block(self, F, pitch=1.0):
        row = np.zeros((F, 2), F32)
        if not self.has_frames:
            return row
        if self.resampled:
            return self._block_resampled(row, F, increment(pitch, self.mix_rate))
        mixed = min(F, self.len - self.pos)
        valid = F if mixed == F else min(F, mixed + LOOKAHEAD)  # valid frames end at 64 + mixed
        si = self.pos - LOOKAHEAD + np.arange(valid)
        ok = si >= self.start
        row[:valid][ok] = self.S[si[ok]]
        self._end(row, F, mixed, valid)
        self.pos += mixed
        return row

    def _block_resampled(self, row, F, inc):
        end_fp = self.len << 16
        mixed = F
        if self.fp_pos >= end_fp:
            mixed = 0
        elif inc > 0:
            mixed = min(F, (end_fp - self.fp_pos + inc - 1) // inc)  # first i with fp_pos + i * inc >= end
        valid = F if mixed == F else min(F, mixed + LOOKAHEAD)
        if valid > LOOKAHEAD:
            row[LOOKAHEAD:valid] = cubic_frames(self.S, self.start, self.fp_pos + np.arange(valid - LOOKAHEAD, dtype=np.int64) * inc)
        if self.prev is not None:
            k = min(valid, LOOKAHEAD)
            row[:k] = cubic_frames(self.S, self.start, self.prev[0] + (F - LOOKAHEAD + np.arange(k, dtype=np.int64)) * self.prev[1])
        self._end(row, F, mixed, valid)
        self.prev = (self.fp_pos, inc)
        self.fp_pos += F * inc  # the engine advances over all requested frames
        return row

    def _end(self, row, F, mixed, valid):
        if mixed != F:
            row[mixed:valid] *= ENV[: valid - mixed, None]
            self.has_frames = False


def lengths(F):
    """(At F = 128, F - 64 and F - 63 are the 64 and 65 already listed.)"""
    return sorted({1, 2, 3, 4, 63, 64, 65, F - 64, F - 63, F - 1, F, F + 1, 2 * F - 64, 2 * F, 2 * F + 63, 3 * F + 200})


def starts(n):
    """0, 1, 63, 64; the last frame; pre-start zeros and fade in one block; clamped to the end (a silent first block
    that ends the playback)."""
    return sorted({s for s in (0, 1, 63, 64, n - 1, n - 10, n, n + 5) if s >= 0})


def cases(F):
    """(length, start_frame): the smallest shapes at which the window logic can go wrong, relative to F."""
    return [(n, s) for n in lengths(F) for s in starts(n)]


def run_to_end(pb, F, pitch=1.0, past=2, limit=400):
    """Yield (callback, row) until `past` callbacks after has_frames cleared."""
    after = 0
    for cb in range(limit):
        ended = not pb.has_frames
        yield cb, pb.block(F, pitch(cb) if callable(pitch) else pitch)
        after += ended
        if after == past:
            return
    raise AssertionError("the playback never ended")
