"""Host statements of the two per-rate entry points, the references of the tests:
  * encode_rates       = wifirx_tx_batch_rates: frame i is tx_ref.encode of PSDU i at encodings[i] with seed i (NUMERICS.md
    rule 16 holds per frame);
  * link_stats_by_rate = wifirx_link_stats_by_rate: link_ref.link_stats on the slots whose reference record is complete with
    encoding e, for e = 0..7, beside the totals."""
import numpy as np

import link_ref
import tx_ref


def default_seeds(n):
    return (np.arange(n) % 127) + 1


def encode_rates(psdus, encodings, seeds=None):
    """PSDUs (list of bytes or uint8 arrays), one encoding and one seed per frame -> list of frames (complex64), each what
    wifirx_tx_batch writes for that frame alone"""
    n = len(psdus)
    encodings = np.broadcast_to(np.asarray(encodings), (n,))
    seeds = default_seeds(n) if seeds is None else np.broadcast_to(np.asarray(seeds), (n,))
    out = []
    for p, e, s in zip(psdus, encodings, seeds):
        row = np.frombuffer(bytes(bytearray(p)), np.uint8)[None]
        out.append(tx_ref.encode(row, int(e), [int(s)])[0])
    return out


def _subset(side, sel):
    return {k: (None if v is None else v[sel]) for k, v in side.items()}


def link_stats_by_rate(rx, ref, max_sym, use_hbits=None):
    """rx, ref as link_ref.link_stats takes them.  Returns (total counts, [8] counts): entry e over the slots whose reference
    record is F_COMPLETE with encoding e."""
    def stats(r, f):      # (link_ref.link_stats takes at least one slot)
        return link_ref.link_stats(r, f, max_sym, use_hbits)[0] if len(f["frames"]) else {k: 0 for k in link_ref.COUNTERS}

    total = stats(rx, ref)
    ff = ref["frames"]
    ref_c = (ff["flags"] & link_ref.F_COMPLETE) != 0
    by_rate = []
    for e in range(8):
        sel = np.nonzero(ref_c & (ff["encoding"] == e))[0]
        by_rate.append(stats(_subset(rx, sel), _subset(ref, sel)))
    return total, by_rate


def check_sums(total, by_rate):
    """the identities of include/wifirx.h between the totals and the eight rates"""
    for e in range(8):
        assert by_rate[e]["frames"] == by_rate[e]["frames_ref"], e
    assert sum(b["frames"] for b in by_rate) == total["frames_ref"]
    for k in link_ref.COUNTERS[1:]:
        assert sum(b[k] for b in by_rate) == total[k], k
