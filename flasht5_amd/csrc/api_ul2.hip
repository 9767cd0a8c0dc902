// libfat5.so: the UL2 span-corruption collator -- raw token rows to sentinel-marked input_ids / labels (ul2_kernels.h).
#include "api_common.h"
#include "ul2_kernels.h"

using namespace fat5;

extern "C" {

size_t fat5_sizeof_ul2_params(void) { return sizeof(fat5_ul2_params); }

int fat5_ul2_collate(const fat5_ul2_params* p, void* stream_) {
  if (!p) return fail(FAT5_EINVAL, "ul2_collate: null params");
  if (p->B < 1 || p->L < 1) return fail(FAT5_EINVAL, "ul2_collate: B %d / L %d (both >= 1)", p->B, p->L);
  if (p->max_length < 1 || p->max_labels_length < 1)
    return fail(FAT5_EINVAL, "ul2_collate: max_length %d / max_labels_length %d (both >= 1)", p->max_length, p->max_labels_length);
  if (p->num_denoisers < 1 || p->num_denoisers > UL2_MAX_DENOISERS)
    return fail(FAT5_EINVAL, "ul2_collate: num_denoisers %d outside [1, %d]", p->num_denoisers, UL2_MAX_DENOISERS);
  if (p->num_sentinels < 1) return fail(FAT5_EINVAL, "ul2_collate: num_sentinels %d (>= 1)", p->num_sentinels);
  if (p->tokens_stride < 0 || p->noise_mask_stride < 0)
    return fail(FAT5_EINVAL, "ul2_collate: tokens_stride %lld / noise_mask_stride %lld (both >= 0)", (long long)p->tokens_stride,
                (long long)p->noise_mask_stride);
  const bool given = p->noise_mask != nullptr;
  if (given != (p->denoiser_in != nullptr))
    return fail(FAT5_EINVAL, "ul2_collate: noise_mask and denoiser_in come together (given-mask mode) or not at all");
  if (int rc = check_ptrs("ul2_collate", {{p->tokens, 8, "tokens", true}, {p->lengths, 4, "lengths", true}, {p->step, 8, "step", !given},
                                          {p->mu, 8, "mu", true}, {p->r, 8, "r", true}, {p->max_spans, 4, "max_spans", true},
                                          {p->tokens_len, 4, "tokens_len", true}, {p->prefix_off, 4, "prefix_off", true},
                                          {p->prefix_ids, 8, "prefix_ids", false}, {p->cum_prop, 4, "cum_prop", true},
                                          {p->denoiser_in, 4, "denoiser_in", false}, {p->input_ids, 8, "input_ids", true},
                                          {p->labels, 8, "labels", true}, {p->attention_mask, 1, "attention_mask", true},
                                          {p->decoder_attention_mask, 1, "decoder_attention_mask", true}, {p->enc_len, 4, "enc_len", true},
                                          {p->dec_len, 4, "dec_len", true}, {p->denoiser, 4, "denoiser", true}, {p->status, 4, "status", true}}))
    return rc;
  Ul2Args a = {};
  a.tokens = p->tokens, a.lengths = p->lengths, a.step = p->step;
  a.mu = p->mu, a.r = p->r, a.max_spans = p->max_spans, a.tokens_len = p->tokens_len;
  a.prefix_off = p->prefix_off, a.prefix_ids = p->prefix_ids, a.cum_prop = p->cum_prop;
  a.noise_mask = p->noise_mask, a.denoiser_in = p->denoiser_in;
  a.input_ids = p->input_ids, a.labels = p->labels;
  a.attention_mask = p->attention_mask, a.decoder_attention_mask = p->decoder_attention_mask;
  a.enc_len = p->enc_len, a.dec_len = p->dec_len, a.denoiser = p->denoiser, a.status = p->status;
  a.tokens_stride = p->tokens_stride, a.noise_mask_stride = p->noise_mask_stride;
  a.eos = p->eos_token_id, a.pad = p->pad_token_id, a.sentinel_first = p->sentinel_first_id;
  a.seed = p->seed;
  a.B = p->B, a.L = p->L, a.max_length = p->max_length, a.max_labels_length = p->max_labels_length;
  a.D = p->num_denoisers, a.num_sentinels = p->num_sentinels, a.random_chunk = p->random_chunk != 0;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(ul2_rows_kernel, dim3((unsigned)p->B), dim3(UL2_THREADS), 0, stream, a);
  if (int rc = launched("ul2_collate rows launch")) return rc;
  hipLaunchKernelGGL(ul2_status_kernel, dim3(1), dim3(UL2_THREADS), 0, stream, a);
  return launched("ul2_collate status launch");
}

}  // extern "C"
