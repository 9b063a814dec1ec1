"""The index map of gas_stream_set_loop (include/gas_amd.h), written down once in numpy.

A looped playback behaves exactly as a plain playback over the unrolled stream U[k] = S[m(k)]:
    k <  b: m(k) = k
    k >= b: t = (k - b) mod P;  FORWARD: P = L, m = b + t;  PINGPONG: P = 2L, m = b + (t < L ? t : 2L - 1 - t)
with b = loop_begin, e = loop_end, L = e - b.  NEW behaviour (no counterpart in the reference)."""
import numpy as np

LOOP_DISABLED = 0
LOOP_FORWARD = 1
LOOP_PINGPONG = 2


def loop_map(k, b, e, mode):
    """m(k) for an integer or an integer array k."""
    k = np.asarray(k, dtype=np.int64)
    if mode == LOOP_DISABLED:
        return k.copy()
    L = e - b
    assert L > 0 and mode in (LOOP_FORWARD, LOOP_PINGPONG)
    P = L if mode == LOOP_FORWARD else 2 * L
    t = np.mod(k - b, P)
    folded = b + np.where(t < L, t, 2 * L - 1 - t)
    return np.where(k < b, k, folded)


def unroll(pcm, b, e, mode, length):
    """The first `length` frames of U (a DISABLED stream unrolls to itself, whatever `length`)."""
    pcm = np.asarray(pcm)
    if mode == LOOP_DISABLED:
        return pcm.copy()
    if e == 0:
        e = pcm.shape[0]
    return np.ascontiguousarray(pcm[loop_map(np.arange(length), b, e, mode)])
