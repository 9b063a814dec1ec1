"""GAS_PCM_QOA (include/gas_amd.h) in plain Python / numpy: the QOA file layout, the decoder, an encoder that emits
valid files, files of random slices and random header state, prefixes of a file, and the decoder states csrc/gas_qoa.h
keeps in front of every 80 frames.  Written from the public QOA specification; test_qoa_reference.py pins it to two
hand-worked examples.

File (big-endian): 'qoaf', u32 samples per channel; per 5120 samples a frame: u8 channels, u24 rate, u16 fsamples,
u16 fsize; per channel history[4] i16 and weights[4] i16; then ceil(fsamples / 20) slices per channel, interleaved by
channel.  A slice is a u64: scale factor in bits 63..60, then 20 residual codes of 3 bits, the first in bits 59..57."""
import struct

import numpy as np

SLICE = 20
CHUNK = 80  # frames per device record (csrc/gas_qoa.h)
FRAME = 5120
SPAN_CHUNKS = 32  # k_sample_qoa.hip: chunks a wave decodes ahead of a row
SPAN_FRAMES = SPAN_CHUNKS * CHUNK
RATE = 48000

MULT = (0.75, -0.75, 2.5, -2.5, 4.5, -4.5, 7.0, -7.0)


def _round_away(x):
    return int(np.sign(x) * np.floor(abs(x) + 0.5))


SCALE = [_round_away((sf + 1) ** 2.75) for sf in range(16)]
DEQ = np.array([[_round_away(s * m) for m in MULT] for s in SCALE], np.int64)
INITIAL_WEIGHTS = (0, 0, -8192, 16384)  # what encoders start from


def _wrap32(x):
    return ((x + 0x80000000) & 0xFFFFFFFF) - 0x80000000


def _wrap16(x):
    return ((x + 0x8000) & 0xFFFF) - 0x8000


def decode_slice(h, w, slice_, n=SLICE):
    """n samples of one slice from state (h, w) (lists of 4, changed in place); also how many predictions wrapped."""
    deq = DEQ[slice_ >> 60].tolist()
    out, wrapped = [], 0
    for k in range(n):
        d = deq[(slice_ >> (57 - 3 * k)) & 7]
        acc = w[0] * h[0] + w[1] * h[1] + w[2] * h[2] + w[3] * h[3]
        acc32 = _wrap32(acc)
        wrapped += acc32 != acc
        s = min(max((acc32 >> 13) + d, -32768), 32767)
        delta = d >> 4
        for i in range(4):
            w[i] = _wrap32(w[i] - delta if h[i] < 0 else w[i] + delta)
        h[:] = h[1:] + [s]
        out.append(s)
    return out, wrapped


def frame_slices(fsamples):
    return (fsamples + SLICE - 1) // SLICE


def frame_bytes(fsamples, channels):
    return 8 + 16 * channels + 8 * frame_slices(fsamples) * channels


def file_bytes(frames, channels):
    full, rest = divmod(frames, FRAME)
    return 8 + full * frame_bytes(FRAME, channels) + (frame_bytes(rest, channels) if rest else 0)


def parse(file):
    """(samples, [(channels, fsamples, fsize, states [ch] of (h, w), slices [slice][ch]) per frame])."""
    b = bytes(np.asarray(file, np.uint8).tobytes()) if not isinstance(file, (bytes, bytearray)) else bytes(file)
    assert b[:4] == b"qoaf"
    (samples,) = struct.unpack_from(">I", b, 4)
    frames, at, done = [], 8, 0
    while done < samples:
        ch = b[at]
        fsamples, fsize = struct.unpack_from(">HH", b, at + 4)
        states = []
        for c in range(ch):
            v = struct.unpack_from(">8h", b, at + 8 + 16 * c)
            states.append((list(v[:4]), list(v[4:])))
        n = frame_slices(fsamples)
        sl = struct.unpack_from(f">{n * ch}Q", b, at + 8 + 16 * ch)
        frames.append((ch, fsamples, fsize, states, [sl[k * ch:(k + 1) * ch] for k in range(n)]))
        at += fsize
        done += fsamples
    assert at == len(b), "trailing or missing bytes"
    return samples, frames


def decode_full(file, carry=False):
    """{"samples": int16 [frames][ch], "weights": the final weights per channel, "wrapped": predictions that wrapped,
    "records": int64 [chunks][ch][8], the state (h, w) in front of every CHUNK frames}.  carry=True is the WRONG decoder
    that keeps its state across frame edges (test_qoa_reference.py shows that the tests would catch it)."""
    samples, frames = parse(file)
    ch = frames[0][0]
    out = np.zeros((samples, ch), np.int16)
    records = np.zeros(((samples + CHUNK - 1) // CHUNK, ch, 8), np.int64)
    weights, wrapped, at = [None] * ch, 0, 0
    state = [None] * ch
    for fch, fsamples, _, states, slices in frames:
        assert fch == ch
        for c in range(ch):
            if not carry or state[c] is None:
                state[c] = (list(states[c][0]), list(states[c][1]))
            h, w = state[c]
            for k, sl in enumerate(slices):
                if k % (CHUNK // SLICE) == 0:
                    records[(at + k * SLICE) // CHUNK, c] = h + w
                n = min(SLICE, fsamples - k * SLICE)
                got, wr = decode_slice(h, w, sl[c], n)
                out[at + k * SLICE:at + k * SLICE + n, c] = got
                wrapped += wr
            weights[c] = list(w)
        at += fsamples
    return {"samples": out, "weights": weights, "wrapped": wrapped, "records": records}


def decode(file, channels, frames):
    """The int16 samples of a file: [frames] (mono) or [frames][2], what the GAS_PCM_S16 twin stream holds."""
    s = decode_full(file)["samples"]
    assert s.shape == (frames, channels)
    return np.ascontiguousarray(s[:, 0] if channels == 1 else s)


def records(file):
    """The chunk states: int64 [chunks][ch][8], history then weights."""
    return decode_full(file)["records"]


def build(samples, channels, frames):
    """File bytes (uint8 array) from frames = [(states [ch] of (h, w), slices [slice][ch])]; a partial last slice is
    masked to its codes (zero padding)."""
    b = bytearray(b"qoaf" + struct.pack(">I", samples))
    at = 0
    for states, slices in frames:
        fsamples = min(FRAME, samples - at)
        assert len(slices) == frame_slices(fsamples)
        b += struct.pack(">BBHHH", channels, RATE >> 16, RATE & 0xFFFF, fsamples, frame_bytes(fsamples, channels))
        for h, w in states:
            b += struct.pack(">8h", *[_wrap16(int(v)) for v in list(h) + list(w)])
        for k, sl in enumerate(slices):
            n = min(SLICE, fsamples - k * SLICE)
            keep = ~((1 << (60 - 3 * n)) - 1) & 0xFFFFFFFFFFFFFFFF
            b += struct.pack(f">{channels}Q", *[int(v) & keep for v in sl])
        at += fsamples
    assert at == samples and len(b) == file_bytes(samples, channels)
    return np.frombuffer(bytes(b), np.uint8)


def random_file(rng, frames, channels):
    """Random slices and random full-range int16 state in every frame header: hostile data, both rails, predictions that
    wrap."""
    out = []
    for at in range(0, frames, FRAME):
        n = frame_slices(min(FRAME, frames - at))
        states = [(rng.integers(-32768, 32768, 4).tolist(), rng.integers(-32768, 32768, 4).tolist()) for _ in range(channels)]
        out.append((states, rng.integers(0, 1 << 64, (n, channels), dtype=np.uint64).tolist()))
    return build(frames, channels, out)


def prefix(file, n):
    """The file of the first n frames, re-headered; its decode is the first n frames of the decode."""
    samples, frames = parse(file)
    assert 0 < n <= samples
    out = []
    for k, (ch, _, _, states, slices) in enumerate(frames):
        if k * FRAME >= n:
            break
        out.append((states, slices[:frame_slices(min(FRAME, n - k * FRAME))]))
    return build(n, ch, out)


def encode_channel(samples):
    """[(state, [slice, ...]) per frame] of one int16 channel: per slice the scale factor with the smallest squared error,
    all 16 tried side by side.  Each frame header stores the weights wrapped to int16 and the encoder goes on from what
    it stored, so its state is the decoder's."""
    x = np.asarray(samples, np.int64)
    h = np.zeros(4, np.int64)
    w = np.array(INITIAL_WEIGHTS, np.int64)
    frames = []
    for at in range(0, len(x), FRAME):
        w = _wrap16(w)
        state = (h.tolist(), w.tolist())
        slices = []
        for s0 in range(at, min(at + FRAME, len(x)), SLICE):
            H = np.repeat(h[None, :], 16, axis=0)  # one row per scale factor
            W = np.repeat(w[None, :], 16, axis=0)
            err = np.zeros(16, np.int64)
            codes = []
            for v in x[s0:s0 + SLICE].tolist():
                p = _wrap32((W * H).sum(axis=1)) >> 13
                code = np.abs((v - p)[:, None] - DEQ).argmin(axis=1)
                d = DEQ[np.arange(16), code]
                s = np.clip(p + d, -32768, 32767)
                err += (v - s) ** 2
                W = _wrap32(W + np.where(H < 0, -(d >> 4)[:, None], (d >> 4)[:, None]))
                H = np.concatenate([H[:, 1:], s[:, None]], axis=1)
                codes.append(code)
            sf = int(err.argmin())
            h, w = H[sf], W[sf]
            word = sf << 60
            for k, code in enumerate(codes):
                word |= int(code[sf]) << (57 - 3 * k)
            slices.append(word)
        frames.append((state, slices))
    return frames


def encode(samples):
    """int16 [frames] or [frames][2] -> file bytes (uint8 array)."""
    s = np.asarray(samples, np.int16)
    s = s[:, None] if s.ndim == 1 else s
    per_ch = [encode_channel(s[:, c]) for c in range(s.shape[1])]
    frames = [([per_ch[c][f][0] for c in range(s.shape[1])], [[per_ch[c][f][1][k] for c in range(s.shape[1])] for k in range(len(per_ch[0][f][1]))]) for f in range(len(per_ch[0]))]
    return build(len(s), s.shape[1], frames)


def malformed(file, channels, frames):
    """{what: file bytes} -- each is to be refused as a stream of `channels` x `frames`: one field of a valid file of
    that stream altered, in the last frame header where it is a frame's."""
    at = 8 + (frames - 1) // FRAME * frame_bytes(FRAME, channels)  # the last frame header
    fsamples, fsize = struct.unpack_from(">HH", bytes(file), at + 4)

    def put(offset, data):
        b = bytearray(bytes(file))
        b[offset:offset + len(data)] = data
        return np.frombuffer(bytes(b), np.uint8)

    return {
        "magic": put(0, b"qoaF"),
        "samples": put(4, struct.pack(">I", frames + 1)),
        "channels": put(at, bytes([3 - channels])),
        "fsamples": put(at + 4, struct.pack(">H", fsamples - 1)),
        "fsize": put(at + 6, struct.pack(">H", fsize + 8)),
    }
