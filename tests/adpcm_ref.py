"""GAS_PCM_IMA_ADPCM (include/gas_amd.h) in numpy: the IMA/DVI ADPCM decoder, the byte packing of the engine's
FORMAT_IMA_ADPCM data for mono and stereo, the checkpoints csrc/gas_internal.h keeps in front of every 32 frames, and an
encoder helper.  test_adpcm_reference.py pins the decoder to Python's audioop, which the project did not write.

Codes: one 4-bit value per frame and channel, an array [frames] (mono) or [frames][2] (stereo) of 0 .. 15.
Bytes: channel c's frame i in byte (i >> 1) * channels + c, low nibble for even i, high nibble for odd i."""
import numpy as np

CHUNK = 32
STEP = np.array([7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], np.int64)
INDEX = np.array([-1, -1, -1, -1, 2, 4, 6, 8], np.int64)
assert len(STEP) == 89


def decode_channel(codes, state=(0, 0), want_states=False):
    """One channel's samples (int16) from its codes, starting at state = (predictor, step_index); with want_states
    also the state in front of every frame and behind the last ([frames + 1][2])."""
    predictor, index = int(state[0]), int(state[1])
    out = np.zeros(len(codes), np.int16)
    states = np.zeros((len(codes) + 1, 2), np.int64)
    for i, n in enumerate(np.asarray(codes, np.int64).tolist()):
        states[i] = predictor, index
        step = int(STEP[index])
        index = min(max(index + int(INDEX[n & 7]), 0), 88)
        diff = step >> 3
        if n & 1:
            diff += step >> 2
        if n & 2:
            diff += step >> 1
        if n & 4:
            diff += step
        predictor = min(max(predictor - diff if n & 8 else predictor + diff, -32768), 32767)
        out[i] = predictor
    states[len(codes)] = predictor, index
    return (out, states) if want_states else out


def pack(codes):
    """Codes [frames] or [frames][2] -> the uint8 data gas_stream_create reads, ((frames + 1) // 2) * channels bytes."""
    c = np.asarray(codes, np.uint8)
    c = c[:, None] if c.ndim == 1 else c
    frames, ch = c.shape
    padded = np.zeros((2 * ((frames + 1) // 2), ch), np.uint8)
    padded[:frames] = c
    return np.ascontiguousarray((padded[0::2] | (padded[1::2] << 4)).reshape(-1))


def unpack(data, channels, frames):
    b = np.asarray(data, np.uint8).reshape(-1, channels)
    c = np.zeros((2 * len(b), channels), np.uint8)
    c[0::2] = b & 15
    c[1::2] = b >> 4
    return c[:frames, 0] if channels == 1 else c[:frames]


def decode(data, channels, frames):
    """The int16 samples of packed data: [frames] (mono) or [frames][2], what the GAS_PCM_S16 twin stream holds."""
    c = unpack(data, channels, frames)
    if channels == 1:
        return decode_channel(c)
    return np.stack([decode_channel(c[:, k]) for k in range(channels)], axis=1)


def checkpoints(codes):
    """(predictor, step_index) in front of every CHUNK frames of one channel: [chunks][2]."""
    return decode_channel(codes, want_states=True)[1][:-1][::CHUNK]


def swap_nibbles(b):
    b = np.frombuffer(bytes(b), np.uint8)
    return ((b << 4) | (b >> 4)).astype(np.uint8)


def encode_channel(samples):
    """Codes of one int16 channel by audioop.lin2adpcm, which packs the first sample of a byte into the high nibble: its
    nibbles are swapped into the engine's order and unpacked."""
    import audioop

    s = np.ascontiguousarray(samples, np.int16)
    even = np.concatenate([s, np.zeros(len(s) & 1, np.int16)])
    data, _ = audioop.lin2adpcm(even.tobytes(), 2, None)
    return unpack(swap_nibbles(data), 1, len(s))


def encode(samples):
    """int16 [frames] or [frames][2] -> codes of the same shape."""
    s = np.asarray(samples, np.int16)
    return encode_channel(s) if s.ndim == 1 else np.stack([encode_channel(s[:, k]) for k in range(s.shape[1])], axis=1)
