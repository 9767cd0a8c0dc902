"""UL2 span corruption on the device (libfat5.so: fat5_ul2_collate): what the reference's `DataCollatorForUL2MLM`
(src/data/data_collator_ul2.py) does to one example per row -- draw a denoiser, cut the example to that denoiser's length, draw a
random span mask, rewrite the example into sentinel-marked `input_ids` / `labels` -- on raw token rows that already live on the
device.  Two launches per call, no host read, graph-replayable; include/fat5.h states exactly what is computed.

    ul2_lengths(max_length, max_labels_length, r, mu, prefix_len)   -> (tokens_length, targets_length), host arithmetic
    UL2Collator(denoisers, proportions, max_length=..., ...)        -> collator(tokens, lengths) -> dict of device tensors
    ul2_collate(tokens, lengths, tables, step, ...)                 -> the functional form underneath

Not covered (the caller's business): the reference's best-fit packing of several examples into one row (it produces no segment
ids, so the packed rows could not be told apart downstream), `causal=True` (the decoder-only layout), `fixed_batch_size`
wrap-padding, and dropping short examples (`min_size_inputs`: a kernel cannot shrink B; filter before the call, or look at
status bit 8).  There is no CPU fallback."""
import ctypes
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib

__all__ = ["ul2_lengths", "ul2_tables", "ul2_collate", "UL2Collator", "UL2Tables", "MAX_TOKENS"]

MAX_TOKENS = 4096      # the longest example a drawn mask covers (the LDS budget of the kernel's key sort)
MAX_DENOISERS = 256
F_ENC_CUT, F_DEC_CUT, F_RAW_TOKEN, F_SHORT = 1, 2, 4, 8
_MASK64 = (1 << 64) - 1


def ul2_lengths(max_length, max_labels_length, r, mu, prefix_len):
    """(tokens_length, targets_length): the longest raw example whose corrupted encoder side -- kept tokens, one sentinel per
    noise span, eos -- still fits into max_length - prefix_len columns, and the length of its decoder side.  Noise tokens and
    spans are counted as the span counts of the collator are, with Python's round (half to even).  r == 0 is the
    sequential (S) denoiser, whose lengths follow from the two maxima alone."""
    room = int(max_length) - int(prefix_len)
    if r == 0.0:
        return int(max_labels_length) - 2 + int(max_length // mu) - 2, room

    def sides(n):
        noise = int(round(n * r))
        spans = int(round(noise / mu))
        return n - noise + spans + 1, noise + spans + 1

    n = room
    while sides(n + 1)[0] <= room:
        n += 1
    enc, dec = sides(n)
    if r == 0.5 and dec > enc:   # (equal sides at half density)
        n, dec = n - 1, dec - 1
    return n, dec


@dataclass
class UL2Tables:
    """the denoisers as the kernel reads them, all on one device"""
    mu: torch.Tensor          # (D,) float64
    r: torch.Tensor           # (D,) float64
    max_spans: torch.Tensor   # (D,) int32
    tokens_len: torch.Tensor  # (D,) int32
    prefix_off: torch.Tensor  # (D + 1,) int32
    prefix_ids: torch.Tensor  # (prefix_off[D],) int64
    cum_prop: torch.Tensor    # (D,) float32

    @property
    def num_denoisers(self):
        return self.mu.numel()


def _sentinel_range(sentinel_first_id, num_sentinels):
    return int(sentinel_first_id) - int(num_sentinels) + 1, int(sentinel_first_id)


def _check_vocab(max_length, max_labels_length, sentinel_first_id, num_sentinels):
    if int(max_length) < 1 or int(max_labels_length) < 1:
        raise ValueError(f"max_length {max_length} / max_labels_length {max_labels_length} must both be at least 1")
    if int(num_sentinels) < 1:
        raise ValueError(f"num_sentinels {num_sentinels} must be at least 1")
    if _sentinel_range(sentinel_first_id, num_sentinels)[0] < 0:
        raise ValueError(f"sentinel ids count down from sentinel_first_id = {sentinel_first_id}: {num_sentinels} of them go below 0")


def _host_tables(denoisers, proportions, max_length, max_labels_length, sentinel_first_id, num_sentinels):
    """every check ul2_tables makes, without a device -> the tables as Python lists"""
    _check_vocab(max_length, max_labels_length, sentinel_first_id, num_sentinels)
    D = len(denoisers)
    if not 1 <= D <= MAX_DENOISERS:
        raise ValueError(f"{D} denoisers: between 1 and {MAX_DENOISERS}")
    if len(proportions) != D:
        raise ValueError(f"{len(proportions)} proportions for {D} denoisers")
    props = [float(x) for x in proportions]
    if any(not x >= 0.0 or x == float("inf") for x in props) or not sum(props) > 0.0:
        raise ValueError(f"proportions {props} must be finite, non-negative and not all zero")
    lo, hi = _sentinel_range(sentinel_first_id, num_sentinels)
    prefixes = []
    for i, dn in enumerate(denoisers):
        mu, r, ms = float(dn["mu"]), float(dn["r"]), int(dn["max_spans"])
        if not mu >= 1.0 or mu == float("inf"):
            raise ValueError(f"denoiser {i}: mu = {mu} must be finite and at least 1")
        if not 0.0 <= r < 1.0:
            raise ValueError(f"denoiser {i}: r = {r} outside [0, 1)")
        if ms < 1:
            raise ValueError(f"denoiser {i}: max_spans = {ms} must be at least 1")
        ids = [int(t) for t in dn.get("prefix_ids", ())]
        for t in ids:
            if lo <= t <= hi:
                raise ValueError(f"denoiser {i}: prefix id {t} lies in the sentinel range [{lo}, {hi}]")
            if t < 0:
                raise ValueError(f"denoiser {i}: negative prefix id {t}")
        prefixes.append(ids)
    longest = max(len(x) for x in prefixes)
    if longest + 1 > int(max_length):
        raise ValueError(f"a prefix of {longest} ids and the eos do not fit into max_length = {max_length}")
    tokens_len = [ul2_lengths(max_length, max_labels_length, float(dn["r"]), float(dn["mu"]), longest)[0] for dn in denoisers]
    if min(tokens_len) < 2:
        raise ValueError(f"tokens_len {tokens_len}: every denoiser needs room for at least 2 tokens (max_length / max_labels_length too small)")
    if max(tokens_len) > MAX_TOKENS:
        raise ValueError(f"tokens_len {tokens_len}: at most {MAX_TOKENS} tokens per example (the LDS budget of the span draw)")
    total, acc, cum = sum(props), 0.0, []
    for x in props:
        acc += x / total
        cum.append(acc)
    off = [0]
    for ids in prefixes:
        off.append(off[-1] + len(ids))
    return dict(mu=[float(dn["mu"]) for dn in denoisers], r=[float(dn["r"]) for dn in denoisers],
                max_spans=[min(int(dn["max_spans"]), 2 ** 31 - 1) for dn in denoisers], tokens_len=tokens_len, prefix_off=off,
                prefix_ids=[x for ids in prefixes for x in ids], cum_prop=cum)


_TABLE_DTYPES = dict(mu=torch.float64, r=torch.float64, max_spans=torch.int32, tokens_len=torch.int32, prefix_off=torch.int32,
                     prefix_ids=torch.int64, cum_prop=torch.float32)


def ul2_tables(denoisers, proportions, *, max_length, max_labels_length, sentinel_first_id, num_sentinels, device):
    """denoisers: a list of dict(mu, r, max_spans, prefix_ids); proportions: one non-negative weight each (normalised here; the
    cumulative sums are formed in double and rounded to fp32).  tokens_len[d] = ul2_lengths(max_length, max_labels_length, r, mu,
    the LONGEST prefix)[0], as the reference sizes them.  ValueError names what is wrong."""
    host = _host_tables(denoisers, proportions, max_length, max_labels_length, sentinel_first_id, num_sentinels)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"the UL2 tables must live on the HIP device, got {dev} (the collator has no CPU fallback)")
    return UL2Tables(**{k: torch.tensor(v, dtype=_TABLE_DTYPES[k]).to(dev) for k, v in host.items()})


def _check_tensor(x, name, shape, dtypes, dev):
    if not torch.is_tensor(x):
        raise ValueError(f"{name} must be a tensor, got {type(x).__name__}")
    if x.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError(f"{name} must live on the HIP device (the collator has no CPU fallback)")
    if dev is not None and x.device != dev:
        raise RuntimeError(f"{name} is on {x.device}, tokens on {dev}")


def ul2_collate(tokens, lengths, tables, step, *, seed, max_length, max_labels_length, sentinel_first_id, num_sentinels, eos_token_id,
                pad_token_id, random_chunk=True, noise_mask=None, denoiser=None):
    """tokens (B, L) int64 with unit column stride (any row stride), lengths (B,) int32, `tables` from ul2_tables, `step` an
    int64 device tensor of one element (read on the device, NOT advanced here) -> dict(input_ids (B, max_length) int64, labels
    (B, max_labels_length) int64 padded with -100, attention_mask, decoder_attention_mask (bool), enc_len, dec_len, denoiser (B,)
    int32, status (4,) int32), all on the device.  noise_mask (B, L) uint8 / bool with denoiser (B,) int32: given-mask mode,
    nothing is drawn.  Two launches, no host read."""
    if not torch.is_tensor(tokens) or tokens.dim() != 2:
        raise ValueError(f"tokens must be a (B, L) tensor, got {tuple(tokens.shape) if torch.is_tensor(tokens) else type(tokens).__name__}")
    B, L = tokens.shape
    if B < 1 or L < 1:
        raise ValueError(f"tokens must have at least one row and one column, got {tuple(tokens.shape)}")
    _check_tensor(tokens, "tokens", (B, L), (torch.int64,), None)
    dev = tokens.device
    if tokens.stride(1) != 1 or tokens.stride(0) < 0:
        raise ValueError(f"tokens must have unit column stride and a non-negative row stride, got strides {tokens.stride()}")
    _check_tensor(lengths, "lengths", (B,), (torch.int32,), dev)
    if not isinstance(tables, UL2Tables):
        raise ValueError("tables must come from ul2_tables")
    if tables.mu.device != dev:
        raise RuntimeError(f"the UL2 tables are on {tables.mu.device}, tokens on {dev}")
    _check_tensor(step, "step", (1,), (torch.int64,), dev)
    _check_vocab(max_length, max_labels_length, sentinel_first_id, num_sentinels)
    if (noise_mask is None) != (denoiser is None):
        raise ValueError("noise_mask and denoiser come together (given-mask mode) or not at all")
    if noise_mask is not None:
        _check_tensor(noise_mask, "noise_mask", (B, L), (torch.uint8, torch.bool), dev)
        _check_tensor(denoiser, "denoiser", (B,), (torch.int32,), dev)
        if noise_mask.stride(1) != 1 or noise_mask.stride(0) < 0:
            raise ValueError(f"noise_mask must have unit column stride and a non-negative row stride, got strides {noise_mask.stride()}")
        denoiser = denoiser.contiguous()
    lengths = lengths.contiguous()
    ML, MD = int(max_length), int(max_labels_length)
    out = {
        "input_ids": torch.empty((B, ML), dtype=torch.int64, device=dev),
        "labels": torch.empty((B, MD), dtype=torch.int64, device=dev),
        "attention_mask": torch.empty((B, ML), dtype=torch.bool, device=dev),
        "decoder_attention_mask": torch.empty((B, MD), dtype=torch.bool, device=dev),
        "enc_len": torch.empty((B,), dtype=torch.int32, device=dev),
        "dec_len": torch.empty((B,), dtype=torch.int32, device=dev),
        "denoiser": torch.empty((B,), dtype=torch.int32, device=dev),
        "status": torch.empty((4,), dtype=torch.int32, device=dev),
    }
    p = _lib.Ul2Params()
    p.B, p.L, p.max_length, p.max_labels_length = B, L, ML, MD
    p.num_denoisers, p.num_sentinels, p.random_chunk = tables.num_denoisers, int(num_sentinels), int(bool(random_chunk))
    p.sentinel_first_id, p.eos_token_id, p.pad_token_id, p.seed = int(sentinel_first_id), int(eos_token_id), int(pad_token_id), int(seed) & _MASK64
    p.tokens, p.tokens_stride, p.lengths, p.step = tokens.data_ptr(), tokens.stride(0), lengths.data_ptr(), step.data_ptr()
    p.mu, p.r, p.max_spans, p.tokens_len = (t.data_ptr() for t in (tables.mu, tables.r, tables.max_spans, tables.tokens_len))
    p.prefix_off, p.cum_prop = tables.prefix_off.data_ptr(), tables.cum_prop.data_ptr()
    p.prefix_ids = tables.prefix_ids.data_ptr() if tables.prefix_ids.numel() else None
    if noise_mask is not None:
        p.noise_mask, p.noise_mask_stride, p.denoiser_in = noise_mask.data_ptr(), noise_mask.stride(0), denoiser.data_ptr()
    for name, t in out.items():
        setattr(p, name, t.data_ptr())
    with _lib.on_device(dev):
        _lib.check(_lib.load().fat5_ul2_collate(ctypes.byref(p), _lib.stream_ptr(dev)), "fat5_ul2_collate")
    return out


class UL2Collator:
    """The reference's UL2 collator, one example per row, on the device.

        collator = UL2Collator(denoisers, proportions, max_length=512, max_labels_length=512, sentinel_first_id=32099,
                               num_sentinels=100, eos_token_id=1, pad_token_id=0, seed=0)
        out = collator(tokens, lengths)                 # tokens (B, L) int64, lengths (B,) int32, both on the device
        loss = model(out["input_ids"], out["labels"], attention_mask=out["attention_mask"],
                     decoder_attention_mask=out["decoder_attention_mask"])
        collator.check(out)                             # the one host read: raises if a row was cut or malformed

    `step` is an int64 device counter the kernel reads; every call advances it with an in-place device add, so a call captured in
    a graph draws new masks at each replay (call once before capturing: the first call uploads the denoiser tables).  With
    noise_mask / denoiser given nothing is drawn.  seed None takes one from torch's CPU generator.  The tables and the counter live
    on the device of the first call's tokens; `tokens_len` lists each denoiser's longest example."""

    def __init__(self, denoisers, proportions, *, max_length, max_labels_length, sentinel_first_id, num_sentinels, eos_token_id,
                 pad_token_id, seed=None, random_chunk=True):
        self.denoisers = [dict(d) for d in denoisers]
        self.proportions = [float(x) for x in proportions]
        self.args = dict(max_length=int(max_length), max_labels_length=int(max_labels_length), sentinel_first_id=int(sentinel_first_id),
                         num_sentinels=int(num_sentinels))
        self.eos_token_id, self.pad_token_id = int(eos_token_id), int(pad_token_id)
        self.random_chunk = bool(random_chunk)
        self.seed = (int(torch.randint(0, 2 ** 62, ()).item()) if seed is None else int(seed)) & _MASK64
        self._tables: Optional[UL2Tables] = None
        self._step: Optional[torch.Tensor] = None
        # (every host check runs here, before a device is touched; the tables are uploaded at the first call)
        self.tokens_len = _host_tables(self.denoisers, self.proportions, **self.args)["tokens_len"]

    def _build(self, dev):
        self._tables = ul2_tables(self.denoisers, self.proportions, device=dev, **self.args)
        self._step = torch.zeros(1, dtype=torch.int64, device=dev)

    @property
    def step(self):
        if self._step is None:   # (asked for before the first call: the current device)
            self._build(torch.device("cuda", torch.cuda.current_device()))
        return self._step

    def __call__(self, tokens, lengths, noise_mask=None, denoiser=None):
        if self._tables is None:
            if not (torch.is_tensor(tokens) and tokens.is_cuda):
                raise RuntimeError("tokens must be a tensor on the HIP device (the collator has no CPU fallback)")
            self._build(tokens.device)
        out = ul2_collate(tokens, lengths, self._tables, self._step, seed=self.seed, eos_token_id=self.eos_token_id,
                          pad_token_id=self.pad_token_id, random_chunk=self.random_chunk, noise_mask=noise_mask, denoiser=denoiser,
                          **self.args)
        self._step.add_(1)
        return out

    def check(self, out):
        """the one host read: RuntimeError with one line per status bit that a row of `out` raised"""
        flags, rows, _, _ = out["status"].tolist()
        if not flags:
            return
        a = self.args
        lo, hi = _sentinel_range(a["sentinel_first_id"], a["num_sentinels"])
        said = []
        if flags & F_ENC_CUT:
            said.append(f"an encoder side was longer than max_length = {a['max_length']} and was cut (its last token forced to eos)")
        if flags & F_DEC_CUT:
            said.append(f"a decoder side was longer than max_labels_length = {a['max_labels_length']} and was cut (its last token forced to eos)")
        if flags & F_RAW_TOKEN:
            said.append(f"a raw token equals pad_token_id = {self.pad_token_id} or lies in the sentinel range [{lo}, {hi}]")
        if flags & F_SHORT:
            said.append("an example has fewer than 2 tokens (its row holds only prefix and eos)")
        raise RuntimeError(f"UL2 collator: {rows} row(s) flagged (status {flags}): " + "; ".join(said))
