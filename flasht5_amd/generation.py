"""KV-cached greedy and sampled generation for `FAT5ForConditionalGeneration` (the reference's `generate`, src/model/modeling_flash_t5.py:648-690,
reruns the whole decoder over every token so far at every step; here each step runs ONE new token through the decoder against
per-layer caches).

    state = model.init_decode_state(input_ids, max_length=32)   # encoder once, cross K / V once per layer
    logits = model.decode_step(state, token_ids)                 # (B, vocab) for the next position; the caches grow by one
    labels = model.generate(input_ids, max_length=32, graph=True)
    labels = model.generate(input_ids, do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=1234, graph=True)

What a step runs: the embedding of the new token, then per decoder block the self-attention (q, k, v projected from the one row,
k and v appended to the layer's cache by the decode kernel, the T5 bias of block 0's `forward_1d()` bottom-right aligned), the
cross-attention against the encoder's K / V, and the feed-forward sub-layer -- the same modules, weights and dtype rules as the
training forward (a bf16 model, or fp32 weights under bf16 autocast).  `cache_seqlens` is one (B,) int32 device tensor shared by
every self-attention cache and incremented on the device at the end of each step; nothing a step reads comes from the host, so
`graph=True` captures one step once and replays it per token.

How the modes below share code: `_decoder_blocks` is the one pass through the decoder blocks (`decode_step` and `decode_chunk`
add their own checks, length increment and head), `_step` is `decode_step` + `_pick` (processors, argmax or sampler, bookkeeping),
`_run_steps` is the one eager / capture / replay loop -- greedy, sampled, beam and speculative decoding hand it their step and
their stop predicate -- and `_prefill_prompt` is the one decoder-prompt prefill.

Sampling (`do_sample=True`) replaces the argmax by `sample_logits` (one HIP launch: temperature, top-k, top-p and a Philox draw
keyed by the call's seed with the token's position, cache_seqlens, as the counter), so it is captured and replayed the same way.

Beam search (`num_beams=k > 1`) runs the encoder and the cross K / V projections once on B rows, shared by the
B * k beam rows through the decode kernel's `cache_batch_idx`; the self-attention caches hold B * k rows and are never copied
or reordered: each beam reads its history through the `cache_row_batch` table of parents, which the beam-step kernel
(flasht5_amd/beam.py) reorders in place with the running and finished sequences.  Decode step plus beam step is one graph.

Logits processors (`repetition_penalty`, `no_repeat_ngram_size`, `min_length`, `suppress_tokens`) are one more HIP
launch between the decode step and the argmax / sampler / beam step (flasht5_amd/logits_process.py): it reads the running
sequences (`labels`, `running_seqs`) and `cache_seqlens` on the device, so the step stays one graph.  With all of them at
their defaults the launch is not made.  The same launch runs the encoder-decoder ones (`encoder_repetition_penalty`,
`encoder_no_repeat_ngram_size`, `bad_words_ids`, `min_new_tokens`, `forced_bos_token_id`, `forced_eos_token_id`): it then also
reads `input_ids` with the encoder lengths and the rows' decoder-prompt lengths on the device.

Decoder prompts (`decoder_input_ids` (B, P)): the first P - 1 prompt tokens go through the decoder in ONE chunk step
(`decode_chunk`: M tokens per row, M key / value rows appended per layer by the chunk decode kernel, causal inside the chunk), the
loop then starts from the prompt's last token.  `decode_chunk` is also the verification step of speculative decoding.

Speculative decoding, greedy or sampled (`assistant_model`; flasht5_amd/speculative.py): a second, cheaper model drafts gamma
tokens per round, one `decode_chunk` step of gamma + 1 rows checks them, and the verification kernel accepts, rolls the per-row
lengths back and does the step's bookkeeping on the device.  Without an assistant none of it runs: the code path above is unchanged.
With `prompt_lookup_num_tokens` (flasht5_amd/prompt_lookup.py) the drafter is no model but ONE launch per round that
searches input_ids and the row's own sequence for the row's last n-gram and proposes what followed it; the same rounds otherwise.

Padding (`attention_mask`, `decoder_attention_mask`): right-padded masks are validated with one host read before an
encoder runs (`check_padding`).  The encoder then sees only each row's valid keys (packed through `flash_attn_varlen_func` under
fat5_rpe and RoPE, the mask folded into the dense bias otherwise), every cross-attention launch gets the row's encoder length as
its `cache_seqlens`, and a ragged decoder prompt is prefilled by one chunk step with per-row `chunk_seqlens`.  All-ones masks and
None take the code path above.

FP8 KV caches (`kv_cache_dtype="fp8"`): the self-attention caches are allocated as e4m3fn bytes plus one fp32 scale
per (row, position, head), the cross-attention K / V are quantised once by `quantize_kv`, and every decode launch reads bytes and
scales and quantises the rows it appends: (D + 4) / (2 D) of the cache bytes, in every mode above.  None: nothing here runs.

FP8 weights (`weight_dtype="fp8"`): the decoder weights a step reads are quantised once per model (flasht5_amd/w8.py)
and the state's steps run `_decoder_blocks_w8` beside `_decoder_blocks`: each projection one `w8_linear` launch with its RMSNorm
in front and its residual add behind, 9 launches per block where the default path makes about 19.  None: nothing here runs.
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch


@dataclass
class DecodeState:
    """Everything a decoding step reads and writes; all of it lives on the device.  `cache_seqlens[b]` is the number of tokens
    already decoded (the length of every self-attention cache before the next append); the batch shares one length."""
    encoder_hidden_states: torch.Tensor
    self_k: List[torch.Tensor]          # per decoder layer (B, capacity, H, D)
    self_v: List[torch.Tensor]
    cross_k: List[torch.Tensor]         # per decoder layer (B, L_enc, H, D)
    cross_v: List[torch.Tensor]
    cache_seqlens: torch.Tensor         # (B,) int32
    position_bias: Optional[Tuple[torch.Tensor, int]]  # the decoder's (rpe1d, R) (T5), or None (RoPE)
    capacity: int
    steps: int = 0                      # decode_step calls so far (host-side: decode_step refuses to run past the capacity)
    cross_batch_idx: Optional[torch.Tensor] = None  # beam search: (B * k,) int32, beam row -> encoder row (b // k)
    row_batch: Optional[torch.Tensor] = None        # beam search: (B * k, capacity) int32 history table (cache_row_batch)
    cross_seqlens: Optional[torch.Tensor] = None    # padded inputs: (B,) / (B * k,) int32 valid encoder keys per decoding row
    # FP8 caches (kv_cache_dtype="fp8"): per decoder layer the fp32 scales (B, capacity | L_enc, H) of the float8_e4m3fn caches
    self_k_scale: Optional[List[torch.Tensor]] = None
    self_v_scale: Optional[List[torch.Tensor]] = None
    cross_k_scale: Optional[List[torch.Tensor]] = None
    cross_v_scale: Optional[List[torch.Tensor]] = None
    w8: Optional[object] = None   # FP8 weights (weight_dtype="fp8"): the model's w8.DecoderW8; the step then runs `_decoder_blocks_w8`

    def scales(self, i):
        """forward_decode's keywords for layer i -> (self-attention's, cross-attention's); empty without FP8 caches"""
        if self.self_k_scale is None:
            return {}, {}
        return (dict(k_scale=self.self_k_scale[i], v_scale=self.self_v_scale[i]),
                dict(k_scale=self.cross_k_scale[i], v_scale=self.cross_v_scale[i]))

    @property
    def position(self):
        """the step's position as a (1,) int64 device tensor (the RoPE table row): the shared length, clamped on the device to the
        capacity (which init_decode_state keeps within the rotary tables), so that no length a caller writes can index past them"""
        return self.cache_seqlens[:1].long().clamp(0, self.capacity - 1)


def _embed(embedding, ids):
    """`embedding` (the model's `shared`, a stack's `embed_tokens`) of the ids, in the dtype the stack's forward gives it"""
    h = embedding(ids)
    if torch.is_autocast_enabled() and h.is_cuda:  # (FAT5Stack.forward's rule)
        h = h.to(torch.get_autocast_dtype("cuda"))
    return h


def check_kv_cache_dtype(kv_cache_dtype, what="generate"):
    """None, or "fp8" / "fp8_e4m3" -> whether the caches are FP8"""
    if kv_cache_dtype is None:
        return False
    if kv_cache_dtype in ("fp8", "fp8_e4m3"):
        return True
    raise ValueError(f"{what}: kv_cache_dtype {kv_cache_dtype!r} (None, 'fp8' or its alias 'fp8_e4m3')")


def _check_supported(model):
    for blk in model.decoder.block:
        blk.self_attention_layer.self_attention.decode_supported()
        blk.cross_attention_layer.cross_attention.decode_supported()


@dataclass
class Padding:
    """a validated right-padded mask: each row's length on the host (what the one host read brought) and on the device"""
    lengths: List[int]
    lengths_dev: torch.Tensor   # (B,) int32
    mask: torch.Tensor          # (B, L) bool


def _mask_shape_ok(name, mask, like, what):
    if not torch.is_tensor(mask) or mask.dim() != 2 or tuple(mask.shape) != tuple(like.shape[:2]):
        raise ValueError(f"{what}: {name} must be a (B, L) = {tuple(like.shape[:2])} tensor like the ids it masks, got "
                         f"{tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__}")
    if mask.dtype.is_floating_point or mask.dtype.is_complex:
        raise ValueError(f"{what}: {name} must be a bool or integer tensor, got {mask.dtype}")


def check_padding(input_ids, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None, what="generate"):
    """Validate the padding masks of a call with ONE host read -> (encoder Padding or None, decoder Padding or None).

    A mask is (B, L) bool or integer, non-zero = valid, right-padded (row b valid at columns [0, len_b), len_b >= 1).  Holes, left
    padding and an empty row raise ValueError.  None and an all-ones mask both give None: the unpadded code path.  An
    already-validated `Padding` passes through unread."""
    masks = []
    for name, mask, ids in (("attention_mask", attention_mask, input_ids), ("decoder_attention_mask", decoder_attention_mask,
                                                                           decoder_input_ids)):
        if mask is None or isinstance(mask, Padding):
            continue
        if ids is None:
            raise ValueError(f"{what}: {name} needs the ids it masks (decoder_input_ids)")
        _mask_shape_ok(name, mask, ids, what)
        masks.append((name, mask.to(input_ids.device) != 0))   # (both masks live where the model runs)
    out = {"attention_mask": attention_mask if isinstance(attention_mask, Padding) else None,
           "decoder_attention_mask": decoder_attention_mask if isinstance(decoder_attention_mask, Padding) else None}
    if masks:
        rows = []
        for _, m in masks:   # per mask: the B lengths, then one flag (1: every row is a prefix of ones)
            n = m.sum(1)
            prefix = (m == (torch.arange(m.shape[1], device=m.device).unsqueeze(0) < n.unsqueeze(1))).all()
            rows += [n, prefix.to(n.dtype).reshape(1)]
        host = torch.cat(rows).tolist()   # the one host read
        for name, m in masks:
            B, L = m.shape
            lens, ok = host[:B], host[B]
            host = host[B + 1:]
            if min(lens) < 1:
                raise ValueError(f"{what}: {name} has an empty row (row {lens.index(min(lens))}): every row needs at least one "
                                 "valid position")
            if not ok:
                raise ValueError(f"{what}: {name} must be right-padded (each row a run of valid positions, then padding): left "
                                 "padding and masks with holes are not supported")
            if min(lens) < L:
                out[name] = Padding(lens, torch.tensor(lens, dtype=torch.int32).to(m.device), m)
    return out["attention_mask"], out["decoder_attention_mask"]


def _packed_encoder(stack, input_ids, pad):
    """the encoder stack over the valid tokens only (fat5_rpe and RoPE): unpad with indices built from the host lengths, every
    self-attention through flash_attn_varlen_func (the T5 generator or rotated q / k / v, positions local to each row), then the
    rows scattered back into a zero (B, L, d_model) tensor"""
    from .flash_attention_v2_bias import flash_attn_varlen_func
    from .rotary import apply_rotary_emb_qkv
    B, L = input_ids.shape
    dev = input_ids.device
    lens = pad.lengths
    idx = torch.cat([torch.arange(n) + b * L for b, n in enumerate(lens)]).to(dev)
    cu = torch.tensor([0] + [sum(lens[:b + 1]) for b in range(B)], dtype=torch.int32).to(dev)
    mx, total = max(lens), sum(lens)
    h = _embed(stack.embed_tokens, input_ids.reshape(-1).index_select(0, idx).unsqueeze(0))   # (1, total, d_model)
    bias = None
    for blk in stack.block:
        sa = blk.self_attention_layer
        att = sa.self_attention
        H, D = att.n_heads, att.key_value_proj_dim
        n = sa.layer_norm(h)
        q, k, v = (w(n).view(total, H, D) for w in (att.Wq, att.Wk, att.Wv))
        rpe1d, radius = None, 0
        if att.rotary:
            cos, sin, cos_k, sin_k = att.pe_encoding.tables(q.device, q.dtype)
            q, k, v = apply_rotary_emb_qkv(q, k, v, cos, sin, cos_k, sin_k, att.pe_encoding.interleaved, cu_seqlens=cu, max_seqlen=mx)
        else:
            if bias is None:
                bias = att.pe_encoding.forward_1d()   # (block 0 owns the generator; the others are handed it)
            rpe1d, radius = bias
        o = flash_attn_varlen_func(q, k, v, cu, cu, mx, mx, False, att.softmax_scale, rpe1d, radius)
        h = h + att.o(o.reshape(1, total, att.inner_dim))
        h = blk.ff_layer(h)
    h = stack.final_layer_norm(h)
    enc = h.new_zeros((B * L, h.shape[-1]))
    enc.index_copy_(0, idx, h[0])
    return enc.view(B, L, -1)


def _masked_bias_encoder(stack, input_ids, pad):
    """the encoder stack under the dense-bias type: block 0's (1, H, L, L) bias with the padded key columns at the dtype's minimum,
    as FlashT5Attention folds a mask in under use_masking, handed to every block; the padded rows of the result are zeroed"""
    B, L = input_ids.shape
    h = _embed(stack.embed_tokens, input_ids)
    att = stack.block[0].self_attention_layer.self_attention
    bias = att.pe_encoding.compute_bias(L, L, device=h.device).to(h.dtype)
    bias = torch.where(pad.mask.view(B, 1, 1, L), bias, torch.finfo(h.dtype).min).contiguous()
    for blk in stack.block:
        h, bias = blk(h, bias, None)
    return stack.final_layer_norm(h).masked_fill(~pad.mask.unsqueeze(-1), 0)


def encode(model, input_ids, pad=None):
    """the encoder's output (B, L, d_model); with a `Padding`, every row's self-attention sees its own valid keys only and the
    padded rows come back as zeros"""
    if pad is None:
        return model.encoder(input_ids)
    att = model.encoder.block[0].self_attention_layer.self_attention
    if att.rotary or att.attention_type == "fat5_rpe":
        return _packed_encoder(model.encoder, input_ids, pad)
    if att.position_encoding_type != "t5":
        raise NotImplementedError(f"attention_mask with position_encoding_type {att.position_encoding_type!r}")
    return _masked_bias_encoder(model.encoder, input_ids, pad)


@torch.no_grad()
def init_decode_state(model, input_ids, max_length, attention_mask=None, num_beams=1, prompt_length=1, kv_cache_dtype=None,
                      weight_dtype=None):
    """Run the encoder, project every decoder layer's cross-attention K / V once and allocate self-attention caches of capacity
    `max_length + prompt_length` (a decoder prompt of `prompt_length` tokens, the start token included, then max_length new ones).
    `attention_mask` (B, L), right-padded, is applied: it is validated with one host read before the encoder runs
    (`check_padding`; a validated `Padding` is taken as it is), the encoder's self-attention sees each row's valid keys only, and
    `cross_seqlens` carries the rows' encoder lengths to every cross-attention launch.  None and an all-ones mask change nothing.
    num_beams > 1: the encoder and the cross K / V stay at B rows; the self-attention caches, the lengths and the history table
    get B * num_beams rows (row b * k + j: beam j of input b).
    kv_cache_dtype="fp8" (alias "fp8_e4m3"): the self-attention caches are float8_e4m3fn bytes with zeroed fp32 scales beside them,
    the cross-attention K / V are quantised once (`quantize_kv`); anything but these and None raises before the encoder runs.
    weight_dtype="fp8" (alias "fp8_e4m3"): the state's steps read the model's FP8 decoder weights
    (`quantize_decoder_weights`, built once per model) through `w8_linear`; checked, like the decoder's dtype and shapes, before
    the encoder runs."""
    fp8 = check_kv_cache_dtype(kv_cache_dtype, "init_decode_state")
    w8 = _check_weight_dtype(model, weight_dtype, "init_decode_state")
    _check_supported(model)
    first = model.decoder.block[0].self_attention_layer.self_attention
    cap = int(max_length) + int(prompt_length)
    if first.rotary and cap > first.pe_encoding.max_sequence_length:
        # (step t reads row t of the rotary tables; the full forward refuses positions past them the same way)
        raise ValueError(f"max_length {max_length}: the cache of {cap} positions exceeds the rotary tables' "
                         f"{first.pe_encoding.max_sequence_length} rows (max_sequence_length); use max_length <= "
                         f"{first.pe_encoding.max_sequence_length - int(prompt_length)}")
    B = input_ids.shape[0]
    Bk = B * int(num_beams)
    pad, _ = check_padding(input_ids, attention_mask, what="init_decode_state")
    enc = encode(model, input_ids, pad)
    dev = enc.device
    # (the projections' dtype: autocast's when it is on, the weights' otherwise -- the dtype of k and v in the training forward)
    dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else model.shared.weight.dtype
    H, D = first.n_heads, first.key_value_proj_dim
    self_k, self_v, cross_k, cross_v = [], [], [], []
    sks, svs, cks, cvs = [], [], [], []
    for blk in model.decoder.block:
        if fp8:
            from .decode import FP8, quantize_kv
            self_k.append(torch.zeros((Bk, cap, H, D), dtype=torch.uint8, device=dev).view(FP8))
            self_v.append(torch.zeros((Bk, cap, H, D), dtype=torch.uint8, device=dev).view(FP8))
            sks.append(torch.zeros((Bk, cap, H), dtype=torch.float32, device=dev))
            svs.append(torch.zeros((Bk, cap, H), dtype=torch.float32, device=dev))
        else:
            self_k.append(torch.zeros((Bk, cap, H, D), dtype=dtype, device=dev))
            self_v.append(torch.zeros((Bk, cap, H, D), dtype=dtype, device=dev))
        k, v = blk.cross_attention_layer.cross_attention.project_kv(enc)
        if fp8:   # (the 16-bit projections are dropped once their bytes and scales exist)
            (k, ks), (v, vs) = quantize_kv(k), quantize_kv(v)
            cks.append(ks)
            cvs.append(vs)
        cross_k.append(k)
        cross_v.append(v)
    pb = None
    if not first.rotary:
        pb = first.pe_encoding.forward_1d()  # (the (H, 2R+1) generator, built once per generate as the training path builds it per step)
    state = DecodeState(enc, self_k, self_v, cross_k, cross_v, torch.zeros((Bk,), dtype=torch.int32, device=dev), pb, cap)
    if fp8:
        state.self_k_scale, state.self_v_scale, state.cross_k_scale, state.cross_v_scale = sks, svs, cks, cvs
    if w8:
        from .w8 import quantize_decoder_weights
        state.w8 = quantize_decoder_weights(model)
    if num_beams > 1:
        state.cross_batch_idx = torch.arange(Bk, dtype=torch.int32, device=dev) // int(num_beams)
        state.row_batch = torch.zeros((Bk, cap), dtype=torch.int32, device=dev)
    if pad is not None:  # (per decoding row: beam row b * k + j reads encoder row b, so it gets that row's length)
        state.cross_seqlens = pad.lengths_dev if num_beams == 1 else pad.lengths_dev.repeat_interleave(int(num_beams))
    return state


def _decoder_blocks(model, state, h, chunk_seqlens=None):
    """hidden states (B, M, d_model) through every decoder block against the caches of `state` (self-attention, which appends the
    M rows, cross-attention, feed-forward) -> (B, M, d_model) before the final norm; the lengths are the caller's to advance"""
    pos = state.position if model.decoder.block[0].self_attention_layer.self_attention.rotary else None
    for i, blk in enumerate(model.decoder.block):
        sa = blk.self_attention_layer
        ssc, csc = state.scales(i)
        h = h + sa.self_attention.forward_decode(sa.layer_norm(h), state.self_k[i], state.self_v[i], state.cache_seqlens,
                                                 position_bias=state.position_bias, position=pos, cache_row_batch=state.row_batch,
                                                 chunk_seqlens=chunk_seqlens, **ssc)
        ca = blk.cross_attention_layer
        h = h + ca.cross_attention.forward_decode(ca.layer_norm(h), state.cross_k[i], state.cross_v[i], None, position=pos,
                                                  cache_batch_idx=state.cross_batch_idx, cross_seqlens=state.cross_seqlens,
                                                  chunk_seqlens=chunk_seqlens, **csc)
        h = blk.ff_layer(h)
    return h


def _check_weight_dtype(model, weight_dtype, what="generate"):
    """None, or "fp8" / "fp8_e4m3" -> whether the step reads FP8 decoder weights; with them the decoder's dtype and shapes are
    checked too (host only: nothing has run yet)"""
    from .w8 import check_decoder_weights, check_weight_dtype
    if not check_weight_dtype(weight_dtype, what):
        return False
    check_decoder_weights(model, what)
    return True


def _decoder_blocks_w8(model, state, h, chunk_seqlens=None):
    """`_decoder_blocks` over the FP8 weights of `state.w8`: per block norm + qkv, self-attention, o + residual,
    norm + q, cross-attention, o + residual, norm + wi, the gated activation, wo + residual -- every projection ONE `w8_linear`
    launch with its RMSNorm in front and its residual add behind"""
    from . import w8 as w8m   # (looked up per call: the entry point can be wrapped)
    from .gated_act import gated_act_packed
    pos = state.position if model.decoder.block[0].self_attention_layer.self_attention.rotary else None
    B, M = h.shape[:2]
    for i, (blk, lw) in enumerate(zip(model.decoder.block, state.w8.layers)):
        sa, ca, ff = blk.self_attention_layer, blk.cross_attention_layer, blk.ff_layer
        ssc, csc = state.scales(i)
        att = sa.self_attention
        H, D, inner = att.n_heads, att.key_value_proj_dim, att.inner_dim
        qkv = w8m.w8_linear(h, *lw.qkv, norm_weight=sa.layer_norm.weight, eps=sa.layer_norm.variance_epsilon)
        q, k, v = (qkv[..., j * inner:(j + 1) * inner].view(B, M, H, D) for j in range(3))
        o = att.attend_decode(q, k, v, state.self_k[i], state.self_v[i], state.cache_seqlens, position_bias=state.position_bias,
                              position=pos, cache_row_batch=state.row_batch, chunk_seqlens=chunk_seqlens, **ssc)
        h = w8m.w8_linear(o, *lw.self_o, residual=h)
        att = ca.cross_attention
        q = w8m.w8_linear(h, *lw.cross_q, norm_weight=ca.layer_norm.weight, eps=ca.layer_norm.variance_epsilon).view(B, M, H, D)
        o = att.attend_decode(q, None, None, state.cross_k[i], state.cross_v[i], None, position=pos,
                              cache_batch_idx=state.cross_batch_idx, cross_seqlens=state.cross_seqlens, chunk_seqlens=chunk_seqlens,
                              **csc)
        h = w8m.w8_linear(o, *lw.cross_o, residual=h)
        g = w8m.w8_linear(h, *lw.wi, norm_weight=ff.layer_norm.weight, eps=ff.layer_norm.variance_epsilon)
        t = gated_act_packed(g, ff.act.act_name) if ff.act.glu else ff.act.act(g)
        h = w8m.w8_linear(t, *lw.wo, residual=h)
    return h


def _blocks(model, state, h, chunk_seqlens=None):
    """the decoder pass of this state: the default loop, or the FP8-weight one"""
    return (_decoder_blocks if state.w8 is None else _decoder_blocks_w8)(model, state, h, chunk_seqlens)


def _head(model, state, h):
    """final norm + lm_head of the rows of h"""
    if state.w8 is None:
        return model.lm_head(model.decoder.final_layer_norm(h))
    from . import w8 as w8m
    ln = model.decoder.final_layer_norm
    return w8m.w8_linear(h, *state.w8.lm_head, norm_weight=ln.weight, eps=ln.variance_epsilon)


@torch.no_grad()
def decode_step(model, state, token_ids):
    """one token per batch row (B,) or (B, 1) through the decoder against the caches -> logits (B, vocab) of the next position;
    the self-attention caches grow by one (cache_seqlens is incremented on the device)"""
    B = state.cache_seqlens.shape[0]
    if state.steps >= state.capacity:
        raise ValueError(f"decode_step: the caches hold {state.capacity} positions and all of them are used (init_decode_state with a "
                         "larger max_length)")
    state.steps += 1
    if state.w8 is not None:
        h = _decoder_blocks_w8(model, state, _embed(model.shared, token_ids.reshape(B, 1)))
        state.cache_seqlens.add_(1)
        return _head(model, state, h)[:, 0]
    h = _decoder_blocks(model, state, _embed(model.shared, token_ids.reshape(B, 1)))
    h = model.decoder.final_layer_norm(h)
    state.cache_seqlens.add_(1)
    return model.lm_head(h)[:, 0]


@torch.no_grad()
def decode_chunk(model, state, token_ids, logits="all", chunk_seqlens=None):
    """M tokens per batch row (B, M) through the decoder against the caches in one step: every self-attention layer appends its M
    key / value rows with the chunk decode kernel (causal inside the chunk, row i at position cache_seqlens + i), and
    cache_seqlens advances by M on the device.  Returns the logits of all M next positions (B, M, vocab) for logits="all", of the
    last one (B, vocab) for "last" (the final norm and lm_head run on that row only), or None for "none" (both are skipped: a
    prefill that only fills the caches).

    `chunk_seqlens` (B,) int32 on the device: a ragged chunk (right-padded token_ids).  Row b brings its first chunk_seqlens[b]
    tokens: only those are appended, cache_seqlens[b] advances by that many, and "last" gathers row b's logits at its own last
    token (on the device); the logits of rows past a row's length mean nothing."""
    if logits not in ("all", "last", "none"):
        raise ValueError(f"decode_chunk: logits {logits!r} ('all', 'last' or 'none')")
    B = state.cache_seqlens.shape[0]
    if token_ids.dim() != 2 or token_ids.shape[0] != B or token_ids.shape[1] < 1:
        raise ValueError(f"decode_chunk: token_ids must be (B, M) = ({B}, M >= 1), got {tuple(token_ids.shape)}")
    if state.row_batch is not None or state.cross_batch_idx is not None:
        raise ValueError("decode_chunk: a beam-search state takes one token per step (the cache maps are per row)")
    M = token_ids.shape[1]
    if state.steps + M > state.capacity:
        raise ValueError(f"decode_chunk: the caches hold {state.capacity} positions, {state.steps} are used and the chunk brings {M} "
                         "(init_decode_state with a larger max_length or prompt_length)")
    if chunk_seqlens is not None:
        if M == 1:
            raise ValueError("decode_chunk: chunk_seqlens needs M > 1 columns (a one-token step has nothing to pad)")
        if (not torch.is_tensor(chunk_seqlens) or chunk_seqlens.dtype != torch.int32 or tuple(chunk_seqlens.shape) != (B,) or
                chunk_seqlens.device != state.cache_seqlens.device):
            raise ValueError(f"decode_chunk: chunk_seqlens must be a ({B},) int32 tensor on {state.cache_seqlens.device}")
    state.steps += M
    h = _blocks(model, state, _embed(model.shared, token_ids), chunk_seqlens)
    state.cache_seqlens.add_(M if chunk_seqlens is None else chunk_seqlens.clamp(0, M))
    if logits == "none":
        return None
    if logits == "last":
        if chunk_seqlens is not None:   # row b's own last token, selected on the device
            at = (chunk_seqlens.long() - 1).clamp(0, M - 1).view(B, 1, 1).expand(B, 1, h.shape[-1])
            return _head(model, state, h.gather(1, at))[:, 0]
        return _head(model, state, h[:, -1:])[:, 0]
    return _head(model, state, h)


def _check_prompt(model, input_ids, decoder_input_ids, num_beams, decoder_attention_mask=None):
    """host-side validation of a decoder prompt -> its length P (1 without one); with a mask the ids under the padding are not
    looked at (the mask's own validation is check_padding's)"""
    if decoder_input_ids is None:
        if decoder_attention_mask is not None:
            raise ValueError("generate: decoder_attention_mask needs decoder_input_ids")
        return 1
    if num_beams > 1:
        raise ValueError("generate: decoder_input_ids with num_beams > 1 is not supported (beam search starts from the start token)")
    p = decoder_input_ids
    if not torch.is_tensor(p) or p.dtype != torch.int64 or p.dim() != 2 or p.shape[1] < 1:
        raise ValueError("generate: decoder_input_ids must be a (B, P) int64 tensor with P >= 1 (the start token included), got "
                         f"{tuple(p.shape) if torch.is_tensor(p) else type(p).__name__}"
                         f"{' ' + str(p.dtype) if torch.is_tensor(p) else ''}")
    if p.shape[0] != input_ids.shape[0]:
        raise ValueError(f"generate: decoder_input_ids holds {p.shape[0]} rows, input_ids {input_ids.shape[0]}")
    if decoder_attention_mask is not None and not isinstance(decoder_attention_mask, Padding):
        _mask_shape_ok("decoder_attention_mask", decoder_attention_mask, p, "generate")
        p = p.masked_fill(decoder_attention_mask.to(p.device) == 0, 0)
    V = model.lm_head.weight.shape[0]
    lo, hi = int(p.min()), int(p.max())
    if lo < 0 or hi >= V:
        raise ValueError(f"generate: decoder_input_ids holds ids outside the vocabulary [0, {V}) (min {lo}, max {hi})")
    if bool((p == 1).any()):
        raise ValueError("generate: decoder_input_ids holds the EOS id 1 (a finished row cannot be continued)")
    return int(p.shape[1])


def _processed(logits, sequences, lengths, proc, log_softmax=False):
    """the logits processors over the rows' running sequences (`proc`: None, or process_logits' keyword arguments with the
    suppressed ids already on the device); lengths: cache_seqlens after the increment, the start token included"""
    if proc is None:
        return logits
    from .logits_process import process_logits
    return process_logits(logits, sequences, lengths, log_softmax=log_softmax, **proc)


def _step(model, state, tok, labels, seen_eos, proc=None, sampling=None):
    """decode_step + `_pick` -- nothing here reads the host, so the same code is captured as it is"""
    _pick(decode_step(model, state, tok), state, tok, labels, seen_eos, proc, sampling)


def _pick(logits, state, tok, labels, seen_eos, proc=None, sampling=None):
    """a step after the decoder: `logits` (B, vocab) of the position cache_seqlens (already incremented) points at.  The
    processors run first (before the warpers, as in HF), then the argmax, or with `sampling` = (temperature, top_k, top_p, seed)
    `sample_logits` on the processed fp32 row; the Philox counter of row b is cache_seqlens[b] (the new token's position), read
    on the device -- so a captured step draws a fresh uniform at every replay.  The token goes to `tok` and to column
    cache_seqlens of `labels` (a device-side index), and rows that produced a 1 are marked in `seen_eos`"""
    logits = _processed(logits, labels, state.cache_seqlens, proc)
    if sampling is None:
        nxt = logits.argmax(-1)
    else:
        from .sampling import sample_logits
        temperature, top_k, top_p, seed = sampling
        nxt = sample_logits(logits, temperature, top_k, top_p, seed=seed, offsets=state.cache_seqlens)
    tok.copy_(nxt)
    col = state.cache_seqlens.long().unsqueeze(1)  # (already incremented: the new token's column)
    labels.scatter_(1, col, nxt.unsqueeze(1))
    seen_eos.logical_or_(nxt == 1)


def _sampling(do_sample, temperature, top_k, top_p, seed):
    """the `sampling` tuple of a call whose warpers are checked already (None when greedy); a missing seed is one draw from
    torch's default CPU generator"""
    if not do_sample:
        return None
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64))
    return (float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF)


def finish_labels(labels, last=None):
    """the reference's ending (:682-688): the last column becomes 1, and everything after each row's first 1 becomes 0.  `last`
    (B,) int64 on the device: each row's own last column (ragged prompts: rows end at different columns)"""
    labels = labels.clone()
    if last is None:
        labels[:, -1] = 1
    else:
        labels.scatter_(1, last.view(-1, 1), 1)
    L = labels.shape[1]
    first = (labels == 1).long().argmax(-1, keepdim=True)
    keep = torch.arange(L, device=labels.device).unsqueeze(0) <= first
    return labels.masked_fill(~keep, 0)


def _beam_step(model, state, tok, bs, opts, proc=None):
    """decode_step + the beam-step kernel: the next tokens go straight into `tok`; the step count is cache_seqlens after the
    increment, read on the device -- nothing here reads the host, so the same code is captured as it is.  With processors the
    B * k running sequences edit log_softmax(logits) and the beam step scores those rows without renormalising (HF's order)"""
    from .beam import beam_step
    max_length, length_penalty, early_stopping = opts
    logits = decode_step(model, state, tok)
    if proc is not None:
        logits = _processed(logits, bs.running_seqs.view(logits.shape[0], -1), state.cache_seqlens, proc, log_softmax=True)
    bs.tokens = tok
    beam_step(logits, bs, state.cache_seqlens, max_length, length_penalty, early_stopping, logits_normalized=proc is not None)


def _beam_generate(model, input_ids, attention_mask, max_length, graph, k, R, length_penalty, early_stopping, return_scores,
                   proc=None, kv_cache_dtype=None, weight_dtype=None):
    from .beam import new_state, keep_going
    B = input_ids.shape[0]
    dev = input_ids.device
    state = init_decode_state(model, input_ids, max_length, attention_mask, num_beams=k, kv_cache_dtype=kv_cache_dtype,
                              weight_dtype=weight_dtype)
    bs = new_state(B, k, int(max_length) + 1, state.capacity, dev)
    proc = _proc_on_device(proc, dev, input_ids, attention_mask, None, k)
    bs.cache_row_batch = state.row_batch  # (one table: the decode kernel reads it, the beam step reorders it)
    tok = torch.zeros((B * k,), dtype=torch.long, device=dev)
    opts = (int(max_length), float(length_penalty), early_stopping)
    _run_steps(lambda: _beam_step(model, state, tok, bs, opts, proc), lambda: not bool(keep_going(bs.status, early_stopping)),
               int(max_length), graph)
    seqs = bs.finished_seqs[:, :R].reshape(B * R, -1)
    T = int(bs.finished_lens[:, :R].max())
    out = seqs[:, :T + 1].clone()
    if return_scores:
        return out, bs.finished_scores[:, :R].reshape(B * R).clone()
    return out


@torch.no_grad()
def generate(model, input_ids, attention_mask=None, max_length=32, graph=False, *, do_sample=False, temperature=1.0, top_k=50,
             top_p=1.0, seed=None, num_beams=1, num_return_sequences=1, length_penalty=1.0, early_stopping=False,
             return_scores=False, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, suppress_tokens=None,
             decoder_input_ids=None, assistant_model=None, num_assistant_tokens=4, return_stats=False,
             decoder_attention_mask=None, kv_cache_dtype=None, prompt_lookup_num_tokens=None, max_matching_ngram_size=2,
             encoder_repetition_penalty=1.0, encoder_no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0,
             forced_bos_token_id=None, forced_eos_token_id=None, weight_dtype=None):
    """Greedy decoding with the reference's algorithm and return value: start token 0, argmax, stop once every row holds a 1
    (one host read per token, as in the reference), then `finish_labels`.  Returns (B, steps + 1) int64.

    do_sample=True draws each token with `sample_logits` instead of the argmax (HF's GenerationConfig defaults: temperature 1,
    top_k 50, top_p 1): row b's token at position t uses the Philox counter t with the row index b, under one seed per call --
    `seed`, or one drawn from torch's default CPU generator when it is None (so torch.manual_seed makes runs reproducible).
    With do_sample=True the arguments are checked on the host before the encoder runs; with do_sample=False they are neither
    checked nor used.

    graph=True captures one decoding step (for this batch and capacity) once in a HIP graph on one stream and replays it per
    token; the first step runs eagerly (it also builds what the step allocates lazily), so both modes run the same kernels with the
    same arguments and give the same tokens.

    num_beams=k in [2, 16]: HF's beam search (transformers 5.x `_beam_search`, one EOS id 1, max_new_tokens = max_length) with `num_return_sequences`, `length_penalty` and `early_stopping` (False, True or "never") as HF means them.
    Returns (B * num_return_sequences, 1 + T) int64: column 0 is the start token 0, then each hypothesis's tokens including its
    EOS, 0 past its end; T is the longest returned hypothesis.  return_scores=True adds HF's `sequences_scores`
    (B * num_return_sequences,) fp32.  The beam arguments are checked on the host before the encoder runs; do_sample=True with
    beams is rejected.  num_beams=1 is the greedy / sampled path above, unchanged.

    Logits processors, as HF means them and in HF's order, in all three modes, eager and graph=True: `repetition_penalty`
    (> 0, 1 = off; the start token counts as seen, as in HF), `no_repeat_ngram_size` (0 = off), `min_length` (EOS is banned while
    the sequence, start token included, is shorter; 0 = off) and `suppress_tokens` (ids that are never produced, e.g. the
    sentinels; a list of ints below the vocabulary size, moved to the device once per call).  Greedy takes the argmax of the
    processed row, sampling hands it to `sample_logits` (processors before warpers), beam search processes log_softmax(logits)
    and does not renormalise.  They are checked on the host before the encoder runs; with every one at its default no launch
    is added and the step is the code path above.  The sequence buffer of a call with processors holds at most 4096 columns
    (max_length <= 4095).

    Six more of HF's processors run in the same launch, in HF's place in the chain (encoder repetition penalty, repetition
    penalty, n-grams, encoder n-grams, bad words, min_length, min_new_tokens, forced BOS, forced EOS, suppress_tokens), in the
    same modes: `encoder_repetition_penalty` (a float > 0, 1.0 = off: the tokens of the row's input_ids are favoured by
    1 / penalty), `encoder_no_repeat_ngram_size` (0 = off: no n-gram of the row's input_ids is copied), `bad_words_ids` (a
    non-empty list of non-empty lists of ids: a sequence's last token is banned once the row ends in its prefix; [[1]] is
    dropped as HF drops it; at most 1024 sequences of 4096 ids, packed to the device once per call), `min_new_tokens` (EOS is
    banned for the first that many NEW tokens, whatever the decoder prompt's length -- per row with ragged prompts),
    `forced_bos_token_id` (the first token after a lone start token; HF's literal rule, so it never fires behind a longer
    decoder prompt) and `forced_eos_token_id` (the token at each row's own last position P_b + max_length - 1).  The encoder
    ids of a row are its input_ids inside its attention_mask -- HF's classes see the padding too; here a padded row decodes what
    it decodes alone -- and a beam reads the ids of its batch row; at most 4096 encoder ids per row.  All are checked on the
    host before the encoder runs; with all ten processor arguments at their defaults no launch and no allocation is added.

    `decoder_input_ids` (B, P) int64, P >= 1: a decoder prompt as HF takes it, the start token included (None is [[0]]).  Up to
    max_length new tokens follow it; the result is (B, P + steps): the prompt, then the new tokens, with the same ending.  The
    first P - 1 prompt tokens fill the caches in one `decode_chunk` step (eagerly, also with graph=True; none with P = 1), then
    the loop above runs from the prompt's last token.  Greedy decoding, sampling and the logits processors work with it; the
    processors see the prompt, as HF's do, and their 4096-column limit and the rotary tables' limit count it.  The prompt is
    checked on the host before the encoder runs: its shape and batch, ids inside the vocabulary, no EOS id 1; with
    num_beams > 1 it is rejected.

    `assistant_model` (a second FAT5ForConditionalGeneration with the same vocabulary size; None: everything above, unchanged):
    speculative decoding (flasht5_amd/speculative.py; with do_sample=True speculative sampling, DESIGN 4.19, see
    below).  The assistant runs its own encoder once on input_ids
    and drafts `num_assistant_tokens` = gamma in [1, 15] tokens per round with gamma + 1 one-token steps; the model checks them in
    one `decode_chunk` step of gamma + 1 rows, and the verification kernel keeps the agreeing prefix plus the model's own next
    token and rolls both models' lengths back, per row, on the device.  One host read per round; graph=True captures one whole
    round (both models, one stream) after the first eager round and replays it.  The result is what the call returns without an
    assistant -- the drafts only decide how many model steps it takes -- up to the rounding of a chunk step against a one-row
    step where two logits are within it.  decoder_input_ids works as above.  return_stats=True returns
    (labels, {"rounds", "drafted", "accepted"}) with host ints: the rounds run, the tokens drafted for unfinished rows and how many
    of them were accepted.  Rejected on the host before either encoder runs: num_beams > 1, any active logits
    processor, num_assistant_tokens outside [1, 15], a vocabulary mismatch, a model the decode path refuses, and RoPE models
    with more than one batch row (rows advance raggedly; the decode path keeps one rotary position for the batch).

    do_sample=True with `assistant_model` or `prompt_lookup_num_tokens`: speculative sampling.  The assistant draws
    its drafts with `sample_logits` under the same warpers and a Philox key of its own (seed ^ 0x9E3779B97F4A7C15), and the
    verification kernel accepts draft d ~ q with probability min(1, p(d) / q(d)), redrawing the first rejected position from
    norm(max(p - q, 0)); the lookup's drafts are taken as one-hot (accepted with probability p(d)).  Every emitted token is
    distributed exactly as the plain sampler's at that position -- the sequences differ from the call without a drafter, their
    law does not -- and with top_k=1 the result is the greedy one.  The seed is handled as in plain sampling; graph=True,
    decoder_input_ids, the padding masks, kv_cache_dtype and return_stats work as in the greedy speculative loop.
    input_ids that are not on the GPU are refused on the host, after every other check and before an encoder runs.

    Padding.  `attention_mask` (B, L) and `decoder_attention_mask` (B, P), bool or integer, right-padded with at
    least one valid position per row, are validated together with ONE host read before any encoder runs; holes, left padding
    and an empty row raise ValueError, None and all-ones masks change nothing.  With `attention_mask` the encoder's
    self-attention and every decoder cross-attention (greedy, sampled, beam, speculative -- both models --, eager and graph=True)
    see only the valid keys of their row, so a row decodes what it decodes alone, unpadded.  With `decoder_attention_mask` row b's
    prompt is its first P_b columns: ONE chunk step prefills all rows (per-row chunk lengths), row b's first new token comes
    from the logits at its own last prompt row, and max_length new tokens follow each row's own prompt; the result is
    (B, P + steps), rows with shorter prompts end earlier and are 0 from there.  Ragged prompts are rejected with RoPE at B > 1
    (one rotary row per batch) and with an assistant model; beam search takes no decoder prompt at all.

    `kv_cache_dtype`: None (the caches in the activation dtype; everything above, unchanged) or "fp8" (alias
    "fp8_e4m3"): every K / V cache of the call -- self-attention and cross-attention, the assistant's too -- is held as
    float8_e4m3fn bytes with one fp32 scale per (row, position, head), (D + 4) / (2 D) of the bytes.  Rows are quantised as they
    are appended, by the decode kernels; the encoder's K / V once.  All modes and graph=True work with it; the tokens can differ
    from the default's where two logits are within the quantisation error.  Any other value raises ValueError before an
    encoder runs.

    `prompt_lookup_num_tokens` = gamma in [1, 15] (HF's name; None: everything above, unchanged -- no launch, no allocation is
    added): speculative decoding without a second model (flasht5_amd/prompt_lookup.py).  Per round ONE launch
    proposes, per row, the gamma tokens that followed the earliest, longest occurrence (up to `max_matching_ngram_size` = N in
    [1, 16] tokens, HF's name) of the row's last n-gram in input_ids -- inside `attention_mask`: padding is never proposed -- or
    in the row's own sequence, the decoder prompt included; the chunk step and the verification kernel are those of
    `assistant_model`, so the result is what the call returns without it, with the same caveat.  graph=True captures one whole
    round after the first eager one; decoder_input_ids, kv_cache_dtype and return_stats work as with an assistant (`drafted`
    counts the tokens the lookup proposed for unfinished rows, `accepted` those of them that became output).  Rejected on the
    host before the encoder runs: an assistant_model beside it, num_beams > 1, any active logits processor, a
    ragged decoder prompt, a non-int or out-of-range prompt_lookup_num_tokens / max_matching_ngram_size, a model the decode
    path refuses, RoPE at B > 1, and a cache beyond the rotary tables.

    `weight_dtype`: None (everything above, unchanged: the same launches, the same bits) or "fp8" (alias "fp8_e4m3"):
    the decoder weights a cached step reads -- self-attention [Wq; Wk; Wv] and o, cross-attention Wq and o, [wi_0; wi_1], wo and
    lm_head, the assistant's too -- are read as float8_e4m3fn bytes with one fp32 scale per output row, quantised once per model
    (`model.quantize_decoder_weights()`; the 16-bit parameters stay, the encoder and the cross-attention Wk / Wv use them).  Every
    projection of a step is then ONE `w8_linear` launch with its RMSNorm in front and its residual add behind.  All modes,
    kv_cache_dtype and graph=True work with it; the tokens can differ from the default's where two logits are within the
    quantisation error.  Refused with ValueError before an encoder runs: any other value, a decoder whose weights are fp32 (or
    of mixed dtypes), and weight shapes outside the kernel's contract (input widths multiples of 64 up to 16384, output widths
    multiples of 8)."""
    check_kv_cache_dtype(kv_cache_dtype)
    _check_weight_dtype(model, weight_dtype)
    from .beam import check_args as check_beam_args
    check_beam_args(num_beams, num_return_sequences, length_penalty, early_stopping, do_sample)
    P = _check_prompt(model, input_ids, decoder_input_ids, num_beams, decoder_attention_mask)
    attention_mask, dec_pad = check_padding(input_ids, attention_mask, decoder_input_ids, decoder_attention_mask)
    if dec_pad is not None:
        if assistant_model is not None:
            raise ValueError("generate: decoder_attention_mask (a ragged decoder prompt) with assistant_model is not supported")
        if prompt_lookup_num_tokens is not None:
            raise ValueError("generate: decoder_attention_mask (a ragged decoder prompt) with prompt_lookup_num_tokens is not supported")
        if model.decoder.block[0].self_attention_layer.self_attention.rotary and input_ids.shape[0] > 1:
            raise ValueError("generate: a ragged decoder prompt with RoPE needs B = 1: the decode path keeps one rotary position "
                             f"for the batch, and the rows of this one start at {dec_pad.lengths}")
    proc = _check_processors(model, max_length, repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, P,
                             encoder_repetition_penalty, encoder_no_repeat_ngram_size, bad_words_ids, min_new_tokens,
                             forced_bos_token_id, forced_eos_token_id, input_ids.shape[-1])
    if do_sample:  # (with beams do_sample is refused above; this is the one check of the warpers, whatever drafts)
        from .sampling import check_args as check_sampling_args
        check_sampling_args(temperature, top_k, top_p)
    if prompt_lookup_num_tokens is not None or assistant_model is not None:
        from .speculative import check_generate_args, check_lookup_generate_args, speculative_generate
        lookup = prompt_lookup_num_tokens is not None
        if lookup:
            check_lookup_generate_args(model, input_ids, max_length, prompt_lookup_num_tokens, max_matching_ngram_size, P, do_sample,
                                       num_beams, proc is not None, assistant_model)
        else:
            check_generate_args(model, assistant_model, input_ids, max_length, num_assistant_tokens, P, do_sample, num_beams,
                                proc is not None)
            _check_weight_dtype(assistant_model, weight_dtype, "generate: assistant_model")
        return speculative_generate(model, assistant_model, input_ids, attention_mask, max_length, graph,
                                    prompt_lookup_num_tokens if lookup else num_assistant_tokens, P, decoder_input_ids,
                                    bool(return_stats), kv_cache_dtype, lookup_ngram=max_matching_ngram_size if lookup else None,
                                    sampling=_sampling(do_sample, temperature, top_k, top_p, seed), weight_dtype=weight_dtype)
    if num_beams > 1:
        return _beam_generate(model, input_ids, attention_mask, max_length, graph, num_beams, num_return_sequences, length_penalty,
                              early_stopping, return_scores, proc, kv_cache_dtype, weight_dtype)
    proc = _proc_on_device(proc, input_ids.device, input_ids, attention_mask, dec_pad)
    sampling = _sampling(do_sample, temperature, top_k, top_p, seed)
    B = input_ids.shape[0]
    dev = input_ids.device
    state = init_decode_state(model, input_ids, max_length, attention_mask, prompt_length=P, kv_cache_dtype=kv_cache_dtype,
                              weight_dtype=weight_dtype)
    labels = torch.zeros((B, state.capacity), dtype=torch.long, device=dev)
    tok = torch.zeros((B,), dtype=torch.long, device=dev)
    seen_eos = torch.zeros((B,), dtype=torch.bool, device=dev)
    steps = 0
    if decoder_input_ids is not None and dec_pad is None:
        _prefill_prompt(decoder_input_ids, P, labels, tok, (model, state))
    elif dec_pad is not None:
        # ragged prompts: every row's whole prompt in ONE chunk step, its first new token from the logits at its own last prompt
        # row; from here on row b sits at column P_b + steps, which the step reads from cache_seqlens on the device
        prompt = decoder_input_ids.to(dev).masked_fill(~dec_pad.mask, 0)
        labels[:, :P] = prompt
        if int(max_length) >= 1:
            _pick(decode_chunk(model, state, prompt, logits="last", chunk_seqlens=dec_pad.lengths_dev), state, tok, labels, seen_eos,
                  proc, sampling)
            steps = 1
    # (the prefill's token is a step like the others: the same stop check, one host read)
    if not (steps and bool(seen_eos.all())):
        steps = _run_steps(lambda: _step(model, state, tok, labels, seen_eos, proc, sampling), lambda: bool(seen_eos.all()),
                           int(max_length), graph, steps)
    if dec_pad is not None and steps:  # (each row ends at its own last column: P_b + steps - 1)
        return finish_labels(labels[:, :steps + P], last=dec_pad.lengths_dev.long() + (steps - 1))
    return finish_labels(labels[:, :steps + P])


def _check_processors(model, max_length, repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, prompt_length=1,
                      encoder_repetition_penalty=1.0, encoder_no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0,
                      forced_bos_token_id=None, forced_eos_token_id=None, encoder_length=1):
    """host-side validation of the logits processors -> None when all of them are off, else process_logits' keyword arguments
    (without the tensors `_proc_on_device` adds)"""
    from .logits_process import MAX_ENCODER_LEN, MAX_SEQ_LEN, active, check_args
    check_args(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, model.lm_head.weight.shape[0], 1,
               encoder_repetition_penalty, encoder_no_repeat_ngram_size, bad_words_ids, min_new_tokens, forced_bos_token_id,
               forced_eos_token_id)
    if not active(repetition_penalty, no_repeat_ngram_size, min_length, suppress_tokens, encoder_repetition_penalty,
                  encoder_no_repeat_ngram_size, bad_words_ids, min_new_tokens, forced_bos_token_id, forced_eos_token_id):
        return None
    if int(max_length) + int(prompt_length) > MAX_SEQ_LEN:
        raise ValueError(f"max_length {max_length}: the logits processors hold at most {MAX_SEQ_LEN} sequence columns "
                         f"(max_length <= {MAX_SEQ_LEN - int(prompt_length)})")
    if (encoder_repetition_penalty != 1.0 or encoder_no_repeat_ngram_size > 0) and int(encoder_length) > MAX_ENCODER_LEN:
        raise ValueError(f"input_ids of {encoder_length} columns: the encoder-side logits processors hold at most {MAX_ENCODER_LEN} "
                         "encoder ids per row")
    return dict(repetition_penalty=float(repetition_penalty), no_repeat_ngram_size=int(no_repeat_ngram_size),
                min_length=int(min_length), eos_token_id=1, suppress_tokens=suppress_tokens,
                encoder_repetition_penalty=encoder_repetition_penalty, encoder_no_repeat_ngram_size=int(encoder_no_repeat_ngram_size),
                bad_words_ids=bad_words_ids, min_new_tokens=int(min_new_tokens), forced_bos_token_id=forced_bos_token_id,
                forced_eos_token_id=forced_eos_token_id, prompt_length=int(prompt_length), max_new_tokens=int(max_length))


def _proc_on_device(proc, device, input_ids=None, enc_pad=None, dec_pad=None, num_beams=1):
    """the suppressed ids and the bad words moved to the device, once per call, and what the step's launch reads besides the
    sequences: the encoder ids with their per-row lengths (`enc_pad`, a Padding or None), the rows per encoder row (num_beams)
    and the per-row decoder-prompt lengths of a ragged prompt (`dec_pad`)"""
    if proc is None:
        return None
    from .logits_process import pack_bad_words, suppress_to_device
    proc = dict(proc, suppress_tokens=suppress_to_device(proc["suppress_tokens"], device),
                bad_words_ids=pack_bad_words(proc["bad_words_ids"], device, proc["eos_token_id"]))
    if proc["encoder_repetition_penalty"] != 1.0 or proc["encoder_no_repeat_ngram_size"] > 0:
        proc.update(encoder_input_ids=input_ids.to(device=device, dtype=torch.int64).contiguous(),
                    encoder_lengths=None if enc_pad is None else enc_pad.lengths_dev, rows_per_encoder_row=int(num_beams))
    if dec_pad is not None:
        proc.update(prompt_lengths=dec_pad.lengths_dev)
    return proc


def _prefill_prompt(decoder_input_ids, P, labels, tok, *decoders):
    """a (B, P) decoder prompt before the loop: the prompt goes into `labels`, its last token into `tok`, and its first P - 1
    tokens fill the caches of every (model, state) pair in `decoders` in ONE chunk step each, without logits (a pair without a
    state, the assistant's when the lookup drafts, is passed over)"""
    prompt = decoder_input_ids.to(labels.device)
    labels[:, :P] = prompt
    tok.copy_(prompt[:, P - 1])
    for model, state in decoders:
        if P > 1 and state is not None:
            decode_chunk(model, state, prompt[:, :P - 1], logits="none")


def _run_steps(step, stopped, max_steps, graph, steps=0):
    """The loop of every mode: `step()` (one token, one beam step, one speculative round; it reads nothing from the host) until
    `stopped()` (the ONE host read per step) or `max_steps`, counting from `steps` -> the steps run.  The first step runs eagerly
    (it also builds what a step allocates lazily); with `graph` the step is then captured once and replayed -- after the stop
    check, so nothing is captured when the first step ends the call."""
    g = None
    try:
        while steps < max_steps:
            if g is not None:
                g.replay()
            else:
                step()
            steps += 1
            if stopped():
                break
            if graph and g is None and steps < max_steps:
                g = _capture_call(step)
    finally:
        del g
    return steps


def _capture_call(fn):
    """fn() captured in a HIP graph (nothing runs during the capture: the state is unchanged)"""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    ac = torch.is_autocast_enabled()
    with torch.cuda.graph(g):  # (torch's capture stream: one stream, no parallel branches)
        if ac:  # (autocast's weight-cast cache must not hand tensors from outside the capture to it)
            with torch.autocast("cuda", dtype=torch.get_autocast_dtype("cuda"), cache_enabled=False):
                fn()
        else:
            fn()
    return g
