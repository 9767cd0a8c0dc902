// libfat5.so: token selection for generation -- sampling, beam search, logits processors, draft verification and the prompt-lookup drafter.
#include "api_common.h"
#include "sample_kernels.h"
#include "beam_kernels.h"
#include "logits_kernels.h"
#include "spec_kernels.h"
#include "spec_sample_kernels.h"
#include "lookup_kernels.h"

using namespace fat5;

namespace {

bool beam_shape_ok(const fat5_beam_params* p) {
  return p->B >= 1 && p->B <= 65535 && p->k >= 2 && p->k <= BEAM_MAX_K && p->V >= 2 && p->V <= SAMPLE_MAX_V;
}

bool spec_shape_ok(const fat5_spec_params* p) {
  return p->B >= 0 && p->B <= 65535 && p->M >= 2 && p->M <= SPEC_MAX_M && p->V >= 1 && p->V <= SPEC_MAX_V;
}
int spec_slices(const fat5_spec_params* p) { return (p->V + SPEC_SLICE - 1) / SPEC_SLICE; }

// the checks fat5_spec_accept and fat5_spec_accept_sampled share (everything but the workspace)
int spec_check(const fat5_spec_params* p, const char* what) {
  if (p->B < 0 || p->B > 65535) return fail(FAT5_EINVAL, "%s: B %d outside [0, 65535]", what, p->B);
  if (p->M < 2 || p->M > SPEC_MAX_M) return fail(FAT5_EINVAL, "%s: M %d outside [2, %d] (gamma + 1)", what, p->M, SPEC_MAX_M);
  if (p->V < 1 || p->V > SPEC_MAX_V) return fail(FAT5_EINVAL, "%s: V %d outside [1, %d]", what, p->V, SPEC_MAX_V);
  if (p->dtype != FAT5_F32 && p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d", what, p->dtype);
  if (p->row_stride < p->V) return fail(FAT5_EINVAL, "%s: row_stride %lld < V %d", what, (long long)p->row_stride, p->V);
  if (p->B > 1 && p->batch_stride < (int64_t)(p->M - 1) * p->row_stride + p->V)
    return fail(FAT5_EINVAL, "%s: batch_stride %lld: the rows of two batch elements overlap", what, (long long)p->batch_stride);
  if (p->draft_stride < p->M - 1) return fail(FAT5_EINVAL, "%s: draft_stride %lld < gamma %d", what, (long long)p->draft_stride, p->M - 1);
  if (p->ncols < 2) return fail(FAT5_EINVAL, "%s: ncols %d (>= 2)", what, p->ncols);
  if (p->labels_stride < p->ncols) return fail(FAT5_EINVAL, "%s: labels_stride %lld < ncols %d", what, (long long)p->labels_stride, p->ncols);
  if (p->eos_token_id < 0) return fail(FAT5_EINVAL, "%s: eos_token_id %d (>= 0)", what, p->eos_token_id);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  return check_ptrs(what, {{p->logits, es, "logits", true}, {p->draft, 8, "draft", true}, {p->cache_seqlens, 4, "cache_seqlens", true},
                           {p->labels, 8, "labels", true}, {p->tok, 8, "tok", true}, {p->seen_eos, 1, "seen_eos", true},
                           {p->draft_seqlens, 4, "draft_seqlens", false}, {p->limit, 4, "limit", false},
                           {p->n_accepted, 4, "n_accepted", false}, {p->n_new, 4, "n_new", false}});
}

SpecArgs spec_args(const fat5_spec_params* p) {
  SpecArgs a = {};
  a.logits = p->logits;
  a.bstride = p->B > 1 ? p->batch_stride : 0;
  a.stride = p->row_stride;
  a.draft = p->draft;
  a.draft_stride = p->draft_stride;
  a.cache_seqlens = p->cache_seqlens;
  a.draft_seqlens = p->draft_seqlens;
  a.labels = p->labels;
  a.labels_stride = p->labels_stride;
  a.tok = p->tok;
  a.seen_eos = p->seen_eos;
  a.limit = p->limit;
  a.n_accepted = p->n_accepted;
  a.n_new = p->n_new;
  a.ws = static_cast<uint64_t*>(p->workspace);
  a.B = p->B, a.M = p->M, a.V = p->V, a.ncols = p->ncols, a.slices = spec_slices(p), a.limit_scalar = p->limit_scalar;
  a.eos = p->eos_token_id;
  a.vec = aligned16(p->logits) && p->row_stride % 8 == 0 && (p->B == 1 || p->batch_stride % 8 == 0);
  return a;
}

// logits rows the warp launch takes: the B * M target rows, and the B * gamma draft rows when draft_logits is given
size_t spec_sample_rows(const fat5_spec_sample_params* p) {
  return (size_t)p->spec.B * p->spec.M + (p->draft_logits ? (size_t)p->spec.B * (p->spec.M - 1) : 0);
}

}  // namespace

extern "C" {

// ---- temperature / top-k / top-p sampling (sample_kernels.h) ----
size_t fat5_sizeof_sample_params(void) { return sizeof(fat5_sample_params); }

int fat5_sample_logits(const fat5_sample_params* p, void* stream_) {
  const char* what = "sample_logits";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->B < 0) return fail(FAT5_EINVAL, "%s: B %d", what, p->B);
  if (p->V < 1 || p->V > SAMPLE_MAX_V) return fail(FAT5_EINVAL, "%s: V %d outside [1, %d]", what, p->V, SAMPLE_MAX_V);
  if (p->dtype != FAT5_F32 && p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d", what, p->dtype);
  if (int rc = check_warpers(what, p->temperature, p->top_k, p->top_p)) return rc;
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  if (p->B > 1 && p->row_stride < p->V) return fail(FAT5_EINVAL, "%s: row_stride %lld < V %d", what, (long long)p->row_stride, p->V);
  if (int rc = check_ptrs(what, {{p->logits, es, "logits", true}, {p->tokens, 8, "tokens", true}})) return rc;
  if (p->offsets && (reinterpret_cast<uintptr_t>(p->offsets) & 3)) return fail(FAT5_EINVAL, "%s: offsets misaligned", what);
  if (p->uniforms && (reinterpret_cast<uintptr_t>(p->uniforms) & 3)) return fail(FAT5_EINVAL, "%s: uniforms misaligned", what);
  if (p->aux && (reinterpret_cast<uintptr_t>(p->aux) & 3)) return fail(FAT5_EINVAL, "%s: aux misaligned", what);
  if (p->B == 0) return FAT5_OK;
  SampleArgs a = {};
  a.logits = p->logits;
  a.stride = p->row_stride;
  a.offsets = p->offsets;
  a.uniforms = p->uniforms;
  a.tokens = p->tokens;
  a.aux = p->aux;
  a.seed = p->seed;
  a.offset = p->offset;
  a.V = p->V;
  a.top_k = p->top_k;
  a.temperature = p->temperature;
  a.top_p = p->top_p;
  a.vec = aligned16(p->logits) && (p->B == 1 || p->row_stride % 8 == 0);
  hipStream_t stream = (hipStream_t)stream_;
  const bool reg = p->V <= SAMPLE_REG_TILES * SAMPLE_TILE;
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (reg) hipLaunchKernelGGL((sample_logits_kernel<DT, SAMPLE_REG_TILES>), dim3(p->B), dim3(SAMPLE_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((sample_logits_kernel<DT, 0>), dim3(p->B), dim3(SAMPLE_THREADS), 0, stream, a);
  });
  return launched("sample_logits launch");
}

// ---- one beam-search step (beam_kernels.h) ----
size_t fat5_sizeof_beam_params(void) { return sizeof(fat5_beam_params); }

size_t fat5_beam_step_workspace_bytes(const fat5_beam_params* p) {
  if (!p || !beam_shape_ok(p)) return 0;
  return align_up((size_t)p->B * p->k * (2 * p->k) * (sizeof(float) + sizeof(int32_t)), 16);
}

int fat5_beam_step(const fat5_beam_params* p, void* stream_) {
  const char* what = "beam_step";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->k < 2 || p->k > BEAM_MAX_K) return fail(FAT5_EINVAL, "%s: num_beams %d outside [2, %d]", what, p->k, BEAM_MAX_K);
  if (p->V < 2 || p->V > SAMPLE_MAX_V) return fail(FAT5_EINVAL, "%s: V %d outside [2, %d]", what, p->V, SAMPLE_MAX_V);
  if (p->B < 1 || p->B > 65535) return fail(FAT5_EINVAL, "%s: B %d outside [1, 65535]", what, p->B);
  if (p->dtype != FAT5_F32 && p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d", what, p->dtype);
  if (p->row_stride < p->V) return fail(FAT5_EINVAL, "%s: row_stride %lld < V %d", what, (long long)p->row_stride, p->V);
  if (p->seq_len < 2 || p->capacity < 1 || (int64_t)p->B * p->k * p->capacity > INT32_MAX ||
      (int64_t)p->B * p->k * p->seq_len > INT32_MAX)
    return fail(FAT5_EINVAL, "%s: seq_len %d (>= 2) / capacity %d (>= 1) outside the int32 tables", what, p->seq_len, p->capacity);
  if (p->max_length < 1) return fail(FAT5_EINVAL, "%s: max_length %d (>= 1)", what, p->max_length);
  if (!std::isfinite(p->length_penalty)) return fail(FAT5_EINVAL, "%s: length_penalty must be finite", what);
  if (p->early_stopping < 0 || p->early_stopping > 2)
    return fail(FAT5_EINVAL, "%s: early_stopping %d (0 False, 1 True, 2 never)", what, p->early_stopping);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  if (int rc = check_ptrs(what, {{p->logits, es, "logits", true}, {p->running_scores, 4, "running_scores", true},
                                 {p->running_seqs, 8, "running_seqs", true}, {p->cache_row_batch, 4, "cache_row_batch", true},
                                 {p->finished_seqs, 8, "finished_seqs", true}, {p->finished_scores, 4, "finished_scores", true},
                                 {p->finished_flags, 1, "finished_flags", true}, {p->finished_lens, 4, "finished_lens", true},
                                 {p->heuristic, 1, "heuristic", true}, {p->status, 4, "status", true}, {p->tokens, 8, "tokens", true},
                                 {p->step, 4, "step", true}}))
    return rc;
  if (int rc = check_workspace(what, p->workspace, p->workspace_bytes, fat5_beam_step_workspace_bytes(p))) return rc;
  BeamArgs a = {};
  a.logits = p->logits;
  a.stride = p->row_stride;
  a.rs = p->running_scores;
  a.run_seq = p->running_seqs;
  a.table = p->cache_row_batch;
  a.fin_seq = p->finished_seqs;
  a.fin_score = p->finished_scores;
  a.fin_flag = p->finished_flags;
  a.fin_len = p->finished_lens;
  a.unsat = p->heuristic;
  a.status = p->status;
  a.tokens = p->tokens;
  a.step = p->step;
  a.B = p->B, a.k = p->k, a.V = p->V, a.K = 2 * p->k, a.Kr = std::min(2 * p->k, p->V);
  a.ws_score = static_cast<float*>(p->workspace);
  a.ws_tok = reinterpret_cast<int32_t*>(a.ws_score + (size_t)p->B * p->k * a.K);
  a.Lseq = p->seq_len, a.cap = p->capacity, a.max_length = p->max_length, a.early = p->early_stopping;
  a.lp = p->length_penalty;
  a.norm = p->logits_normalized != 0;
  a.vec = aligned16(p->logits) && p->row_stride % 8 == 0;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 rows(p->B * p->k);
  dispatch_dtype(p->dtype, [&](auto dt_) {
    hipLaunchKernelGGL((beam_topk_kernel<decltype(dt_)::value>), rows, dim3(BEAM_TOPK_THREADS), 0, stream, a);
  });
  if (int rc = launched("beam_step top-k launch")) return rc;
  hipLaunchKernelGGL(beam_update_kernel, dim3(p->B), dim3(BEAM_THREADS), 0, stream, a);
  return launched("beam_step update launch");
}

// ---- logits processors (logits_kernels.h) ----
size_t fat5_sizeof_logits_params(void) { return sizeof(fat5_logits_params); }

int fat5_process_logits(const fat5_logits_params* p, void* stream_) {
  const char* what = "process_logits";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->rows < 0) return fail(FAT5_EINVAL, "%s: rows %d", what, p->rows);
  if (p->V < 2 || p->V > LOGITS_MAX_V) return fail(FAT5_EINVAL, "%s: V %d outside [2, %d]", what, p->V, LOGITS_MAX_V);
  if (p->dtype != FAT5_F32 && p->dtype != FAT5_F16 && p->dtype != FAT5_BF16) return fail(FAT5_EINVAL, "%s: dtype %d", what, p->dtype);
  if (p->row_stride < p->V) return fail(FAT5_EINVAL, "%s: row_stride %lld < V %d", what, (long long)p->row_stride, p->V);
  if (p->out_stride < p->V) return fail(FAT5_EINVAL, "%s: out_stride %lld < V %d", what, (long long)p->out_stride, p->V);
  if (p->seq_len < 1 || p->seq_len > LOGITS_MAX_SEQ) return fail(FAT5_EINVAL, "%s: seq_len %d outside [1, %d]", what, p->seq_len, LOGITS_MAX_SEQ);
  if (p->seq_stride < p->seq_len) return fail(FAT5_EINVAL, "%s: seq_stride %lld < seq_len %d", what, (long long)p->seq_stride, p->seq_len);
  if (!std::isfinite(p->repetition_penalty) || !(p->repetition_penalty > 0.f))
    return fail(FAT5_EINVAL, "%s: repetition_penalty %g (finite and > 0)", what, (double)p->repetition_penalty);
  if (p->no_repeat_ngram_size < 0) return fail(FAT5_EINVAL, "%s: no_repeat_ngram_size %d (>= 0)", what, p->no_repeat_ngram_size);
  if (p->min_length < 0) return fail(FAT5_EINVAL, "%s: min_length %d (>= 0)", what, p->min_length);
  if (p->eos_token_id < 0 || p->eos_token_id >= p->V) return fail(FAT5_EINVAL, "%s: eos_token_id %d outside [0, V)", what, p->eos_token_id);
  if (p->n_suppress < 0 || p->n_suppress > LOGITS_MAX_SUPPRESS)
    return fail(FAT5_EINVAL, "%s: n_suppress %d outside [0, %d]", what, p->n_suppress, LOGITS_MAX_SUPPRESS);
  const size_t es = p->dtype == FAT5_F32 ? 4 : 2;
  if (int rc = check_ptrs(what, {{p->logits, es, "logits", true}, {p->out, 4, "out", true}, {p->sequences, 8, "sequences", true},
                                 {p->lengths, 4, "lengths", true}}))
    return rc;
  if (p->n_suppress > 0)
    if (int rc = check_ptrs(what, {{p->suppress_tokens, 4, "suppress_tokens", true}})) return rc;
  const bool inplace = static_cast<const void*>(p->out) == p->logits;
  if (inplace && (p->dtype != FAT5_F32 || p->out_stride != p->row_stride))
    return fail(FAT5_EINVAL, "%s: in place (out == logits) needs fp32 logits and out_stride == row_stride", what);
  // ---- the appended fields (all zero / NULL: the call as it was) ----
  const double phi = p->encoder_repetition_penalty;
  if (!std::isfinite(phi) || phi < 0.0) return fail(FAT5_EINVAL, "%s: encoder_repetition_penalty %g (finite and > 0; 0 or 1: off)", what, phi);
  const bool enc_pen = phi != 0.0 && phi != 1.0;
  if (p->encoder_no_repeat_ngram_size < 0)
    return fail(FAT5_EINVAL, "%s: encoder_no_repeat_ngram_size %d (>= 0)", what, p->encoder_no_repeat_ngram_size);
  const bool enc_on = enc_pen || p->encoder_no_repeat_ngram_size > 0;
  if (enc_on) {
    if (!p->encoder_input_ids || (reinterpret_cast<uintptr_t>(p->encoder_input_ids) & 7))
      return fail(FAT5_EINVAL, "%s: encoder_input_ids: null or misaligned pointer with an encoder processor on", what);
    if (p->encoder_len < 1 || p->encoder_len > LOGITS_MAX_ENC)
      return fail(FAT5_EINVAL, "%s: encoder_len %d outside [1, %d]", what, p->encoder_len, LOGITS_MAX_ENC);
    if (p->encoder_stride < p->encoder_len)
      return fail(FAT5_EINVAL, "%s: encoder_stride %lld < encoder_len %d", what, (long long)p->encoder_stride, p->encoder_len);
    if (p->encoder_lengths && (reinterpret_cast<uintptr_t>(p->encoder_lengths) & 3)) return fail(FAT5_EINVAL, "%s: encoder_lengths: misaligned pointer", what);
    if (p->rows_per_encoder_row < 1 || p->encoder_rows < 1 || (int64_t)p->encoder_rows * p->rows_per_encoder_row < p->rows)
      return fail(FAT5_EINVAL, "%s: %d encoder_rows of %d rows_per_encoder_row do not cover %d rows", what, p->encoder_rows,
                  p->rows_per_encoder_row, p->rows);
  }
  if (p->n_bad_words < 0 || p->n_bad_words > LOGITS_MAX_BAD_WORDS)
    return fail(FAT5_EINVAL, "%s: n_bad_words %d outside [0, %d]", what, p->n_bad_words, LOGITS_MAX_BAD_WORDS);
  if (p->n_bad_words > 0) {
    if (p->n_bad_word_ids < p->n_bad_words || p->n_bad_word_ids > LOGITS_MAX_BAD_IDS)
      return fail(FAT5_EINVAL, "%s: n_bad_word_ids %d outside [n_bad_words, %d]", what, p->n_bad_word_ids, LOGITS_MAX_BAD_IDS);
    if (int rc = check_ptrs(what, {{p->bad_words_ids, 4, "bad_words_ids", true}, {p->bad_words_offsets, 4, "bad_words_offsets", true}})) return rc;
    if (const int32_t* o = p->bad_words_offsets_host) {  // the host's copy of the offsets: checked here, before the launch
      if (o[0] != 0 || o[p->n_bad_words] != p->n_bad_word_ids)
        return fail(FAT5_EINVAL, "%s: bad_words_offsets run from %d to %d, not from 0 to n_bad_word_ids %d", what, o[0], o[p->n_bad_words], p->n_bad_word_ids);
      for (int i = 0; i < p->n_bad_words; ++i)
        if (o[i + 1] <= o[i]) return fail(FAT5_EINVAL, "%s: bad_words_offsets not increasing at %d (%d, %d)", what, i, o[i], o[i + 1]);
    }
  }
  if (p->min_new_tokens < 0) return fail(FAT5_EINVAL, "%s: min_new_tokens %d (>= 0)", what, p->min_new_tokens);
  if (p->forced_tokens & ~(FAT5_FORCED_BOS | FAT5_FORCED_EOS)) return fail(FAT5_EINVAL, "%s: forced_tokens %d", what, p->forced_tokens);
  if ((p->forced_tokens & FAT5_FORCED_BOS) && (p->forced_bos_token_id < 0 || p->forced_bos_token_id >= p->V))
    return fail(FAT5_EINVAL, "%s: forced_bos_token_id %d outside [0, V)", what, p->forced_bos_token_id);
  if ((p->forced_tokens & FAT5_FORCED_EOS) && (p->forced_eos_token_id < 0 || p->forced_eos_token_id >= p->V))
    return fail(FAT5_EINVAL, "%s: forced_eos_token_id %d outside [0, V)", what, p->forced_eos_token_id);
  if ((p->forced_tokens & FAT5_FORCED_EOS) && p->max_new_tokens < 1)
    return fail(FAT5_EINVAL, "%s: max_new_tokens %d (>= 1 with a forced EOS)", what, p->max_new_tokens);
  if (p->min_new_tokens > 0 || (p->forced_tokens & FAT5_FORCED_EOS)) {
    if (p->prompt_lengths ? (reinterpret_cast<uintptr_t>(p->prompt_lengths) & 3) != 0 : p->prompt_length < 1)
      return fail(FAT5_EINVAL, "%s: prompt_lengths misaligned, or NULL with prompt_length %d (>= 1)", what, p->prompt_length);
  }
  const bool ext = enc_on || p->n_bad_words > 0 || p->min_new_tokens > 0 || p->forced_tokens != 0;
  if (p->rows == 0) return FAT5_OK;
  LogitsArgs a = {};
  a.logits = p->logits;
  a.stride = p->row_stride;
  a.out = p->out;
  a.out_stride = p->out_stride;
  a.seq = p->sequences;
  a.seq_stride = p->seq_stride;
  a.lengths = p->lengths;
  a.suppress = p->n_suppress > 0 ? p->suppress_tokens : nullptr;
  a.V = p->V, a.seq_len = p->seq_len, a.ngram = p->no_repeat_ngram_size, a.min_length = p->min_length, a.eos = p->eos_token_id;
  a.n_suppress = p->n_suppress;
  a.log_softmax = p->log_softmax != 0;
  a.copy = !inplace || a.log_softmax;
  a.penalty = p->repetition_penalty;
  a.vec = aligned16(p->logits) && p->row_stride % 8 == 0;
  a.vec_out = aligned16(p->out) && p->out_stride % 4 == 0;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(p->rows);
  size_t lds = 0;
  if (ext) {  // the instance with the encoder-side processors, bad words, min_new_tokens and the forced tokens
    a.enc = enc_on ? p->encoder_input_ids : nullptr;
    a.enc_stride = p->encoder_stride;
    a.enc_lengths = p->encoder_lengths;
    a.enc_len = enc_on ? p->encoder_len : 0;
    a.rows_per_enc = p->rows_per_encoder_row;
    a.enc_ngram = p->encoder_no_repeat_ngram_size;
    a.enc_penalty = enc_pen ? (float)(1.0 / p->encoder_repetition_penalty) : 1.f;  // (HF: 1 / phi in double, used as an fp32 scalar)
    a.bad_ids = p->bad_words_ids, a.bad_off = p->bad_words_offsets, a.n_bad = p->n_bad_words, a.n_bad_ids = p->n_bad_word_ids;
    a.min_new = p->min_new_tokens, a.prompt_length = p->prompt_length, a.prompt_lengths = p->prompt_lengths;
    a.max_new = p->max_new_tokens;
    a.forced_bos = (p->forced_tokens & FAT5_FORCED_BOS) ? p->forced_bos_token_id : -1;
    a.forced_eos = (p->forced_tokens & FAT5_FORCED_EOS) ? p->forced_eos_token_id : -1;
    lds = (size_t)((a.enc_len + LOGITS_ENC_PAD - 1) & ~(LOGITS_ENC_PAD - 1)) * sizeof(int32_t);
  }
  dispatch_dtype(p->dtype, [&](auto dt_) {
    constexpr int DT = decltype(dt_)::value;
    if (ext) hipLaunchKernelGGL((process_logits_kernel<DT, true>), grid, dim3(LOGITS_THREADS), lds, stream, a);
    else hipLaunchKernelGGL((process_logits_kernel<DT, false>), grid, dim3(LOGITS_THREADS), 0, stream, a);
  });
  return launched("process_logits launch");
}

// ---- draft verification of speculative greedy decoding (spec_kernels.h) ----
size_t fat5_sizeof_spec_params(void) { return sizeof(fat5_spec_params); }

size_t fat5_spec_accept_workspace_bytes(const fat5_spec_params* p) {
  if (!p || !spec_shape_ok(p)) return 0;
  return align_up((size_t)p->B * p->M * spec_slices(p) * sizeof(uint64_t), 16);
}

int fat5_spec_accept(const fat5_spec_params* p, void* stream_) {
  const char* what = "spec_accept";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (int rc = spec_check(p, what)) return rc;
  if (p->B == 0) return FAT5_OK;
  if (int rc = check_workspace(what, p->workspace, p->workspace_bytes, fat5_spec_accept_workspace_bytes(p))) return rc;
  const SpecArgs a = spec_args(p);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(p->B * p->M, a.slices);
  dispatch_dtype(p->dtype, [&](auto dt_) {
    hipLaunchKernelGGL((spec_argmax_kernel<decltype(dt_)::value>), grid, dim3(SPEC_THREADS), 0, stream, a);
  });
  if (int rc = launched("spec_accept argmax launch")) return rc;
  hipLaunchKernelGGL(spec_accept_kernel, dim3(p->B), dim3(64), 0, stream, a);
  return launched("spec_accept launch");
}

// ---- draft verification of speculative sampling (spec_sample_kernels.h) ----
size_t fat5_sizeof_spec_sample_params(void) { return sizeof(fat5_spec_sample_params); }

size_t fat5_spec_accept_sampled_workspace_bytes(const fat5_spec_sample_params* p) {
  if (!p || !spec_shape_ok(&p->spec)) return 0;
  return align_up(spec_sample_rows(p) * SPEC_SAMPLE_WORDS * sizeof(uint64_t), 16);
}

int fat5_spec_accept_sampled(const fat5_spec_sample_params* p, void* stream_) {
  const char* what = "spec_accept_sampled";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  const fat5_spec_params* g = &p->spec;
  if (int rc = spec_check(g, what)) return rc;
  if (int rc = check_warpers(what, p->temperature, p->top_k, p->top_p)) return rc;
  const size_t es = g->dtype == FAT5_F32 ? 4 : 2;
  if (p->draft_logits) {
    if (reinterpret_cast<uintptr_t>(p->draft_logits) % es) return fail(FAT5_EINVAL, "%s: draft_logits: misaligned pointer", what);
    if (p->draft_row_stride < g->V)
      return fail(FAT5_EINVAL, "%s: draft_row_stride %lld < V %d", what, (long long)p->draft_row_stride, g->V);
    if (g->B > 1 && p->draft_batch_stride < (int64_t)(g->M - 2) * p->draft_row_stride + g->V)
      return fail(FAT5_EINVAL, "%s: draft_batch_stride %lld: the rows of two batch elements overlap", what, (long long)p->draft_batch_stride);
  }
  if (int rc = check_ptrs(what, {{p->uniforms, 4, "uniforms", false}, {p->sampled, 8, "sampled", false}, {p->aux, 4, "aux", false}})) return rc;
  if (g->B == 0) return FAT5_OK;
  if (int rc = check_workspace(what, g->workspace, g->workspace_bytes, fat5_spec_accept_sampled_workspace_bytes(p))) return rc;
  SpecSampleArgs a = {};
  a.s = spec_args(g);
  a.draft_logits = p->draft_logits;
  a.dl_bstride = g->B > 1 ? p->draft_batch_stride : 0;
  a.dl_stride = p->draft_row_stride;
  a.uniforms = p->uniforms;
  a.sampled = p->sampled;
  a.aux = p->aux;
  a.seed = p->seed;
  a.offset = p->offset;
  a.top_k = p->top_k;
  a.temperature = p->temperature;
  a.top_p = p->top_p;
  a.dl_vec = p->draft_logits && aligned16(p->draft_logits) && p->draft_row_stride % 8 == 0 && (g->B == 1 || p->draft_batch_stride % 8 == 0);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 rows((unsigned)spec_sample_rows(p));
  const bool reg = g->V <= SAMPLE_REG_TILES * SAMPLE_TILE;
  return dispatch_dtype(g->dtype, [&](auto dt_) -> int {
    constexpr int DT = decltype(dt_)::value;
    if (reg) hipLaunchKernelGGL((spec_warp_kernel<DT, SAMPLE_REG_TILES>), rows, dim3(SAMPLE_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((spec_warp_kernel<DT, 0>), rows, dim3(SAMPLE_THREADS), 0, stream, a);
    if (int rc = launched("spec_accept_sampled warp launch")) return rc;
    hipLaunchKernelGGL((spec_sample_accept_kernel<DT>), dim3(g->B), dim3(SAMPLE_THREADS), 0, stream, a);
    return launched("spec_accept_sampled launch");
  });
}

// ---- prompt-lookup drafting of speculative greedy decoding (lookup_kernels.h) ----
size_t fat5_sizeof_lookup_params(void) { return sizeof(fat5_lookup_params); }

int fat5_lookup_draft(const fat5_lookup_params* p, void* stream_) {
  const char* what = "lookup_draft";
  if (!p) return fail(FAT5_EINVAL, "%s: null params", what);
  if (p->B < 0 || p->B > 65535) return fail(FAT5_EINVAL, "%s: B %d outside [0, 65535]", what, p->B);
  if (p->L_src < 0 || p->L_src > LOOKUP_MAX_LEN) return fail(FAT5_EINVAL, "%s: L_src %d outside [0, %d]", what, p->L_src, LOOKUP_MAX_LEN);
  if (p->ncols < 1 || p->ncols > LOOKUP_MAX_LEN) return fail(FAT5_EINVAL, "%s: ncols %d outside [1, %d]", what, p->ncols, LOOKUP_MAX_LEN);
  if (p->gamma < 1 || p->gamma > LOOKUP_MAX_GAMMA) return fail(FAT5_EINVAL, "%s: gamma %d outside [1, %d]", what, p->gamma, LOOKUP_MAX_GAMMA);
  if (p->max_ngram < 1 || p->max_ngram > LOOKUP_MAX_NGRAM)
    return fail(FAT5_EINVAL, "%s: max_ngram %d outside [1, %d]", what, p->max_ngram, LOOKUP_MAX_NGRAM);
  if (p->V < 0) return fail(FAT5_EINVAL, "%s: V %d (>= 0; 0: no id is cut)", what, p->V);
  if (p->source_stride < p->L_src) return fail(FAT5_EINVAL, "%s: source_stride %lld < L_src %d", what, (long long)p->source_stride, p->L_src);
  if (p->labels_stride < p->ncols) return fail(FAT5_EINVAL, "%s: labels_stride %lld < ncols %d", what, (long long)p->labels_stride, p->ncols);
  if (p->draft_stride < p->gamma) return fail(FAT5_EINVAL, "%s: draft_stride %lld < gamma %d", what, (long long)p->draft_stride, p->gamma);
  if (int rc = check_ptrs(what, {{p->source, 8, "source", p->L_src > 0}, {p->labels, 8, "labels", true},
                                 {p->cache_seqlens, 4, "cache_seqlens", true}, {p->tok, 8, "tok", true}, {p->seen_eos, 1, "seen_eos", true},
                                 {p->draft, 8, "draft", true}, {p->src_seqlens, 4, "src_seqlens", false},
                                 {p->n_proposed, 4, "n_proposed", false}}))
    return rc;
  if (p->B == 0) return FAT5_OK;
  LookupArgs a = {};
  a.source = p->source;
  a.source_stride = p->source_stride;
  a.src_seqlens = p->src_seqlens;
  a.labels = p->labels;
  a.labels_stride = p->labels_stride;
  a.cache_seqlens = p->cache_seqlens;
  a.tok = p->tok;
  a.seen_eos = p->seen_eos;
  a.draft = p->draft;
  a.draft_stride = p->draft_stride;
  a.n_proposed = p->n_proposed;
  a.L_src = p->L_src, a.ncols = p->ncols, a.gamma = p->gamma, a.N = p->max_ngram, a.V = p->V;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(lookup_draft_kernel, dim3(p->B), dim3(LOOKUP_THREADS), 0, stream, a);
  return launched("lookup_draft launch");
}

}  // extern "C"
