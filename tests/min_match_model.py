"""numpy model of the counting any clause of term_masks_kernel
(bm25mi_termmask.hip), shared by tests/test_min_match_host.py (CPU) and
tests/test_gpu_min_match.py.  It restates the plane arithmetic the kernel
runs on every mask word: a bit-sliced counter of P = bit_length(need) planes
that starts at 2^P - need, a ripple add of each term's bitmap word, and the
carry out of the top plane ORed into a sticky ``reached`` word — the documents
whose count has reached ``need``.  Planes are uint32 arrays, one element per
mask word, as the kernel keeps one register per plane and word."""
import numpy as np

PLANES = 16  # kCountPlanes: need <= B <= 65535


def planes_of(need: int) -> int:
    return int(need).bit_length()


def counter_init(need: int, words: int):
    """(planes [P, words] uint32, reached [words] uint32) before any term."""
    P = planes_of(need)
    assert 1 <= P <= PLANES, need
    init = (1 << P) - need
    cnt = np.zeros((P, words), np.uint32)
    for p in range(P):
        if (init >> p) & 1:
            cnt[p] = 0xFFFFFFFF
    return cnt, np.zeros(words, np.uint32)


def counter_add(cnt, reached, word):
    """One term's bitmap words added in place: carry = plane & b; plane ^= b."""
    carry = np.asarray(word, np.uint32).copy()
    for p in range(cnt.shape[0]):
        c = cnt[p] & carry
        cnt[p] ^= carry
        carry = c
    reached |= carry


def reached_after(need: int, words_seq):
    """The sticky word after adding every bitmap of words_seq [n, words]."""
    words_seq = np.asarray(words_seq, np.uint32)
    cnt, reached = counter_init(need, words_seq.shape[1])
    for w in words_seq:
        counter_add(cnt, reached, w)
    return reached

