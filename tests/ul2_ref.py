"""Host restatement of the UL2 collator's contract (include/fat5.h `fat5_ul2_collate`) in plain loops, for the UL2
tests.  Only the Philox words are vectorised (tests/dropout_ref.philox4x32_10_np); everything else is written the way the
contract words it, one row and one position at a time.  Tables are the host lists of `flasht5_amd.ul2._host_tables`."""
import numpy as np

from dropout_ref import philox4x32_10_np

MAX_TOKENS = 4096
MASK = 0xFFFFFFFF


def words(c0, row, stream, step, seed):
    """W(c0, stream) of the contract for an array (or scalar) of c0 -> four uint32 arrays"""
    seed = int(seed) & ((1 << 64) - 1)
    c0 = np.asarray(c0, dtype=np.uint64)
    return philox4x32_10_np((c0, np.uint64(row), np.uint64(stream), np.uint64(int(step) & MASK)), (seed & MASK, seed >> 32))


def span_counts(n, mu, r, max_spans, num_sentinels):
    """(noise, spans) of a span denoiser; Python's round on a float is round-half-to-even, as rint"""
    noise = min(max(int(round(n * r)), 1), n - 1)
    spans = max(1, min(max_spans, num_sentinels, int(round(noise / mu)), noise, n - noise))
    return noise, spans


def segmentation(items, parts, row, stream, step, seed):
    """part lengths of the uniform composition of `items` into `parts` positive parts"""
    cnt = items - 1
    if parts == 1:
        return [items]
    i = np.arange(cnt, dtype=np.uint64)
    w = words(i >> np.uint64(2), row, stream, step, seed)
    keys = []
    for j in range(cnt):
        keys.append((int(w[j & 3][j]) << 32) | j)
    cuts = sorted(k & MASK for k in sorted(keys)[:parts - 1])
    lengths, last = [], 0
    for c in cuts:          # a cut at c starts a new part at item c + 1
        lengths.append(c + 1 - last)
        last = c + 1
    lengths.append(items - last)
    return lengths


def draw_mask(n, mu, r, max_spans, num_sentinels, row, step, seed):
    """the drawn noise mask of n >= 2 tokens as a list of bools, and (noise, spans) (None for the S-denoiser)"""
    if max_spans == 1:
        head = int(round(n / mu))
        return [i >= head for i in range(n)], None
    noise, spans = span_counts(n, mu, r, max_spans, num_sentinels)
    a = segmentation(noise, spans, row, 1, step, seed)
    b = segmentation(n - noise, spans, row, 2, step, seed)
    mask = []
    for k in range(spans):
        mask += [False] * b[k] + [True] * a[k]
    assert len(mask) == n
    return mask, (noise, spans)


def streams(t, mask, eos, sentinel_first):
    """the contract's walk -> (encoder stream, decoder stream) as lists of ints"""
    enc, dec = [], []
    enc_sentinels = dec_sentinels = 0
    for i in range(len(t)):
        if i == 0 or mask[i] != mask[i - 1]:
            if mask[i]:
                enc.append(sentinel_first - enc_sentinels)
                enc_sentinels += 1
            else:
                dec.append(sentinel_first - dec_sentinels)
                dec_sentinels += 1
        if int(t[i]) != eos:
            (dec if mask[i] else enc).append(int(t[i]))
    return enc, dec


def collate(tokens, lengths, tab, *, seed, step, max_length, max_labels_length, sentinel_first_id, num_sentinels, eos_token_id,
            pad_token_id, random_chunk=True, noise_mask=None, denoiser=None):
    """tokens (B, L) and lengths (B,) numpy arrays, tab the host tables -> dict of numpy arrays as the device returns them, plus
    `counts`: per row (noise, spans) or None"""
    tokens = np.asarray(tokens)
    B, L = tokens.shape
    D = len(tab["mu"])
    cum = [np.float32(x) for x in tab["cum_prop"]]
    out = dict(input_ids=np.full((B, max_length), pad_token_id, dtype=np.int64), labels=np.full((B, max_labels_length), -100, dtype=np.int64),
               attention_mask=np.zeros((B, max_length), dtype=bool), decoder_attention_mask=np.zeros((B, max_labels_length), dtype=bool),
               enc_len=np.zeros(B, dtype=np.int32), dec_len=np.zeros(B, dtype=np.int32), denoiser=np.zeros(B, dtype=np.int32))
    flags_any, flagged, counts = 0, 0, []
    lo_sent = sentinel_first_id - num_sentinels + 1
    for b in range(B):
        nb = min(max(int(lengths[b]), 0), L)
        flags, start, n = 0, 0, nb
        if noise_mask is not None:
            d = min(max(int(denoiser[b]), 0), D - 1)
        else:
            w = words(0, b, 0, step, seed)
            u = np.float32(int(w[0]) >> 8) * np.float32(2.0 ** -24)
            d = D - 1
            for i in range(D):
                if u < cum[i]:
                    d = i
                    break
            tl = min(max(int(tab["tokens_len"][d]), 0), MAX_TOKENS)
            if nb > tl:
                start = (int(w[1]) * (nb - tl)) >> 32 if random_chunk else 0
                n = tl
        cnt = None
        if n < 2:
            flags |= 8
            t, mask = [], []
        else:
            t = [int(x) for x in tokens[b, start:start + n]]
            if noise_mask is not None:
                mask = [bool(x) for x in noise_mask[b, :n]]
            else:
                mask, cnt = draw_mask(n, tab["mu"][d], tab["r"][d], tab["max_spans"][d], num_sentinels, b, step, seed)
        counts.append(cnt)
        if any(x == pad_token_id or lo_sent <= x <= sentinel_first_id for x in t):
            flags |= 4
        enc, dec = streams(t, mask, eos_token_id, sentinel_first_id)
        enc = list(tab["prefix_ids"][tab["prefix_off"][d]:tab["prefix_off"][d + 1]]) + enc + [eos_token_id]
        dec = dec + [eos_token_id]
        if len(enc) > max_length:
            flags |= 1
            enc = enc[:max_length - 1] + [eos_token_id]
        if len(dec) > max_labels_length:
            flags |= 2
            dec = dec[:max_labels_length - 1] + [eos_token_id]
        out["input_ids"][b, :len(enc)] = enc
        out["labels"][b, :len(dec)] = dec
        out["attention_mask"][b, :len(enc)] = True
        out["decoder_attention_mask"][b, :len(dec)] = True
        out["enc_len"][b], out["dec_len"][b], out["denoiser"][b] = len(enc), len(dec), d
        flags_any |= flags
        flagged += flags != 0
    out["status"] = np.array([flags_any, flagged, out["enc_len"].max(), out["dec_len"].max()], dtype=np.int32)
    out["counts"] = counts
    return out
