// Engine internals shared by dd_engine.hip and the measurement hooks in dd_tools.hip (libdropdec_tools.so only).
#pragma once
#include <string.h>

#include <vector>

#include "dd_lm_kernels.h"

#define MAX_MEMBERS DD_MAX_MEMBERS
#define GROUP_ROWS 72     // rows of the widest decode pass: the members of eight sequences + eight un-masked rows riding along (nine operand planes)
#define GROUP_PLANES (GROUP_ROWS / 8)
#define GROUP_MAX_LANES 64
#define KV_ROWS 64        // new K/V rows kept per layer: 16 members, or the base rows of up to 64 lanes (group step)
#define MAX_NEW_TOKENS 8192

// the LM's weight matrices: the four of a layer, and the lm_head (dd_weight below describes them — the ONE place that does)
enum { DD_M_QKV = 0, DD_M_O, DD_M_GATE_UP, DD_M_DOWN, DD_M_LM_HEAD };
struct LayerW {
  u32x4_t* w[4] = {nullptr, nullptr, nullptr, nullptr};   // packed tiles, by DD_M_*
  float* s[4] = {nullptr, nullptr, nullptr, nullptr};     // fp8: per-row scales, packed order; MXFP4: u32 block-scale words
  float *norm1, *norm2;
};

struct dd_lm {
  dd_lm_config cfg;
  int d, dff, V, Vpad, H, Hkv, q_dim, kv_dim, Lyr, T_cap, Lmax;
  int S_d, S_q, S_ff, qkv_tiles, q_tiles, k_tiles;
  std::vector<void*> allocs;
  size_t bytes = 0;
  unsigned long long serial = 0;
  dd_lm* wsrc = nullptr;       // lane created by dd_lm_create_shared: weights (and rope tables) belong to this handle
  float* grp_logits = nullptr; // [GROUP_MAX_LANES][Vpad] base-pass logits of a group step (this handle is the group's first lane)
  int32_t* grp_argmax = nullptr;
  // rider (group_step_rider): the un-masked row of this sequence's NEXT step, computed ahead while it rode in another group's member
  // sweep — logits / argmax parked here until the step they belong to starts; valid while pend_step == steps_since_prefill
  float* base_next = nullptr;
  int32_t* argmax_next = nullptr;
  bool pend_valid = false;
  int pend_step = -1;
  DDState* chunk_states = nullptr;   // [32] positions of the rows of a short prompt chunk (dd_lm_prefill_extend)
  float *chunk_k = nullptr, *chunk_v = nullptr;   // [32][kv_dim] roped K / V rows of the chunk, one layer at a time
  const float *commit_k = nullptr, *commit_v = nullptr;   // K == 0 group step: this lane's base row in the leader's scratch
  // weights
  std::vector<LayerW> lw;
  u32x4_t* lm_head = nullptr;
  float* s_lm = nullptr;
  int wq = 0;                  // weight storage: 0 16-bit, 1 OCP e4m3fn + per-row scales (DD_WQ_FP8), 2 OCP MXFP4 (DD_WQ_MXFP4)
  int wf = 0;                  // 16-bit weight / operand type: 0 bf16, 1 fp16 (weight_format 2: fp16 checkpoints stay exact)
  int kv16 = 0;                // KV cache storage: 0 fp32, 1 fp16 (the reference's cache width; layouts in dd_lm_kernels.h)
  u32x4_t* deq_tmp = nullptr;  // fp8 / MXFP4: bf16 tiles of ONE matrix for the prefill GEMM
  float* final_norm = nullptr;
  uint16_t* embed = nullptr;
  float *rope_cos = nullptr, *rope_sin = nullptr;
  // kv
  float *kc = nullptr, *vc = nullptr;
  size_t lsk = 0, lsv = 0;
  // decode scratch
  float *xa, *qbuf, *knew, *vnew, *ssq_a, *ssq_b, *part_o, *part_ml, *hidden;
  int32_t* spec_ok = nullptr;   // speculative step: 1 = the members of the combined sweep stand, 0 = re-run them (device flag)
  uint32_t* rng_backup = nullptr;   // mt19937 state before the speculative draws (the re-run repeats exactly these)
  float* gemv_part = nullptr;   // partial sums of the slice-resident 16 / 32-row GEMVs (dd_gemv_slices.h)
  size_t gemv_part_floats = 0;
  u32x4_t *xop_d, *xop_q, *xop_ff;
  float *base_logits, *member_logits, *last_logits, *last_hidden;
  int member_rows_cap = 0;    // rows member_logits holds: 16 at creation, DD_MAX_MEMBERS from the first step with K > 16 on (ensure_member_rows)
  int32_t *argmax_base, *member_tok, *member_vote, *tokens;
  uint8_t *keep, *drop, *drop_bits, *leak_bits;
  int32_t* n_drop;
  DDState* state;
  // prefill scratch
  float *px, *pq, *image_logits;
  uint16_t *p1_hi, *p1_lo, *p2_hi, *p2_lo;
  // scratch of dd_lm_prefill_group (weight owner only): n * seq_rows rows of residual, q, and the two operand plane pairs
  SeqTab* seq_tab = nullptr;    // device table of a dd_lm_prefill_group call led by this handle
  size_t pb_rows = 0;
  float *pb_x = nullptr, *pb_q = nullptr;
  uint16_t *pb1_hi = nullptr, *pb1_lo = nullptr, *pb2_hi = nullptr, *pb2_lo = nullptr;
  int32_t* row_index;
  float *epi, *alea, *var, *scalars, *topk_vals, *kl_ws;
  int32_t* topk_ids;
  void* unc_ws;
  size_t unc_ws_bytes;
  double* kv_sums;
  // host mirrors
  int T_host = 0, span_start = 0, L = 0, n_tok_host = 0, last_K = 0;
  bool prefilled = false;
  bool have_leak = false;
  int bit0 = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // hipGraph cache of whole decode steps (key: K, probabilities, key-tile count, rng)
  struct GraphEntry {
    unsigned long long key;
    hipGraphExec_t exec;
  };
  std::vector<GraphEntry> graphs;
  int steps_since_prefill = 0;
  // host-visible token mirror (pinned, device-mapped): the decode loop can watch for EOS without synchronising
  int32_t* tok_host = nullptr;       // host pointer: [0] = count, [1..] = tokens
  int32_t* tok_host_dev = nullptr;   // the same memory as seen from the device
  int spec_seq_host = 0;             // speculation checks announced to the host so far (dd_lm_decode_step_sync)
  // speculation policy of this sequence (dd_lm_set_speculation): -1 the process default, 0 never, 1 always, 2 adaptive —
  // dd_lm_decode_step_sync learns every check's verdict and stops speculating while too few of them hold
  int spec_mode = -1;
  float spec_rate = 1.0f;            // running share of speculative steps that held (weight 1/8 per step)
  int spec_cooldown = 0;             // adaptive: two-sweep steps left before speculation is tried again
  long long spec_n[4] = {0, 0, 0, 0};   // speculative steps that held / were re-run, two-sweep steps, switches to two-sweep
  // further branches of a group step (the group's first lane owns them): the member sweeps are dealt over the caller's stream
  // and these, and run concurrently
  hipStream_t side[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
  float *part_o_ride = nullptr, *part_ml_ride = nullptr;   // flash-decoding partials of the riding rows (their attention shares a launch with the members')
  // tensor-parallel shard (dd_tp.hip): this handle holds the q/k/v/gate/up columns and the o/down rows of rank tp_rank of
  // tp_world (its dims above are the LOCAL ones); the row-parallel matrices write partial sums into this rank's slot of the
  // gather buffer [tp_world][rows][d] and every rank adds the slots in rank order
  int tp_world = 1, tp_rank = 0;
  float* tp_gather = nullptr;        // linked ranks of one process share rank 0's buffer; one rank per process: its own
  size_t tp_gather_floats = 0;
  int (*tp_exchange)(void* ctx, int rows, void* stream) = nullptr;   // one rank per process: all-gather of the slots (torch.distributed)
  void* tp_ctx = nullptr;
  // generation record (dd_lm_set_record, dd_record.hip): the caller's ring of `rec_cap` records and, optionally, its score plane
  void* rec = nullptr;
  int rec_cap = 0;
  float* rec_scores = nullptr;
  size_t rec_scores_ld = 0;
};

// pieces of dd_engine.hip that the tensor-parallel driver (dd_tp.hip) reuses
int dd_engine_prefill_head(dd_lm* h, const int32_t* row_index, int n_rows, float* logits, hipStream_t st, const float* src);
int dd_engine_prefill_tail(dd_lm* h, const float* x_rows, int T0, int span_start, int span_len, hipStream_t st);
int dd_engine_step_keep(dd_lm* h, const int32_t* gate, hipStream_t st);
int dd_engine_step_begin(dd_lm* h, hipStream_t st);          // k_step_begin: the step's RoPE position
void dd_engine_bump_epoch();                 // every tuning call: graph keys carry the epoch, a step captured under other settings is not replayed
unsigned long long dd_engine_epoch();
int dd_engine_tp_alloc(dd_lm* h, float** p, size_t floats);  // device memory owned (and released) by the handle
// set by libdropdec_tools.so (dd_tools_trace_*): called at the end of every group_finish, on the stream of that sweep
extern int (*dd_engine_group_finish_hook)(dd_lm* const* qs, int ng, int K, hipStream_t st);
// generation record (dd_record.hip): one record per listed sequence, one workgroup each.  mode DD_REC_STEP: a decode step, between
// the vote and the step's end (slot = the sequence's token count, nothing for a finished sequence); DD_REC_FIRST: slot 0 after a
// prefill's greedy token (no ensemble); DD_REC_FIRST_ENSEMBLE: slot 0 after dd_lm_prefill_ensemble's vote.  Sequences without an
// attached record are left out; no launch when none has one.
#define DD_REC_STEP 0
#define DD_REC_FIRST 1
#define DD_REC_FIRST_ENSEMBLE 2
int dd_record_launch(dd_lm* const* qs, int n, int K, int mode, hipStream_t st);
// one packed sweep of nb rows through all layers + lm_head (dd_engine.hip)
int lm_sweep(dd_lm* h, int nb, const uint8_t* bits, int row0, float* logits_out, hipStream_t st, dd_lm* const* lanes = nullptr,
             const int32_t* skip_if = nullptr);

// -----------------------------------------------------------------------------------------------
// One description of a weight matrix.  Allocation sizes, the synthetic fill, the loaders' destinations and the W / scale / S /
// n_tiles of every GEMV and GEMM launch come from dd_weight(); nothing else spells out a matrix's geometry.
// -----------------------------------------------------------------------------------------------
struct WMat {
  u32x4_t* W;      // packed tiles in the handle's storage kind (h->wq)
  float* scale;    // fp8: one float per packed row; MXFP4: one u32 per row and 128 k; 16-bit storage: nullptr
  int S;           // K / 32
  int n_tiles;     // 16-row tiles (gate/up: gate and up tiles interleaved)
};
// which: DD_M_*; `layer` is ignored for DD_M_LM_HEAD.  A lane sees its owner's matrices (h->lw / h->lm_head are copies of the owner's).
static inline WMat dd_weight(const dd_lm* h, int layer, int which) {
  if (which == DD_M_LM_HEAD) return {h->lm_head, h->s_lm, h->S_d, h->Vpad / 16};
  const LayerW& w = h->lw[layer];
  const int S[4] = {h->S_d, h->S_q, h->S_d, h->S_ff};
  const int n_tiles[4] = {h->qkv_tiles, h->d / 16, 2 * h->dff / 16, h->d / 16};
  return {w.w[which], w.s[which], S[which], n_tiles[which]};
}
// u32x4_t units of the tiles: a tile row holds S * 64 of them in 16-bit storage, half that in fp8, a quarter in MXFP4
static inline size_t dd_weight_units(const dd_lm* h, const WMat& m) {
  return (size_t)m.n_tiles * m.S * 64 / (h->wq == DD_WQ_MXFP4 ? 4 : (h->wq ? 2 : 1));
}
// entries of `scale` (fp8: floats, MXFP4: u32 words of four e8m0 bytes)
static inline size_t dd_weight_scales(const dd_lm* h, const WMat& m) {
  return (size_t)m.n_tiles * 16 * (h->wq == DD_WQ_MXFP4 ? m.S / 4 : 1);
}

// -----------------------------------------------------------------------------------------------
// Decode: the GemvArgs of the five launches of a layer sweep, filled with what every sweep agrees on.  The caller adds what is its
// own: nb / n_groups / nb_rider / half_planes, state / state_rows, knew / vnew / *_g, out / out_g, skip_if, part / part_floats.
// -----------------------------------------------------------------------------------------------
// matrix source and operand only (the row-parallel launches of a tensor-parallel shard stop here: dd_tp.hip)
static inline GemvArgs dd_gemv_matrix(const dd_lm* h, const WMat& m, const u32x4_t* xop) {
  GemvArgs a;
  memset(&a, 0, sizeof(a));
  a.wf = h->wf, a.wq = h->wq;
  a.W = m.W, a.wscale = m.scale, a.S = m.S, a.n_tiles = m.n_tiles, a.xop = xop;
  return a;
}
// the operand is the un-normalised row: its rstd comes from ssq_n partial sums of squares per row
static inline void dd_gemv_norm_in(GemvArgs& a, const dd_lm* h, const float* ssq_in, int ssq_n) {
  a.ssq_in = ssq_in, a.ssq_n = ssq_n, a.ssq_ld = h->d / 16, a.inv_k = 1.0f / h->d, a.eps = h->cfg.rms_eps;
}
// EPI_RESID into the residual rows; the next GEMV's operand is normalised with normw_next, its sums of squares go to ssq_out
static inline void dd_gemv_resid_out(GemvArgs& a, const dd_lm* h, const float* normw_next, float* ssq_out) {
  a.out = h->xa, a.ldo = h->d, a.normw_next = normw_next, a.xop_next = h->xop_d, a.S_next = h->S_d;
  a.ssq_out = ssq_out, a.ssq_ld = h->d / 16;
}
static inline GemvArgs dd_gemv_qkv(const dd_lm* h, int layer, int ssq_n) {   // ssq_n: 1 after the embedding, d / 16 after a layer
  GemvArgs a = dd_gemv_matrix(h, dd_weight(h, layer, DD_M_QKV), h->xop_d);
  dd_gemv_norm_in(a, h, h->ssq_a, ssq_n);
  a.qbuf = h->qbuf, a.q_tiles = h->q_tiles, a.k_tiles = h->k_tiles, a.q_dim = h->q_dim, a.kv_dim = h->kv_dim;
  a.rope_cos = h->rope_cos, a.rope_sin = h->rope_sin;
  return a;
}
static inline GemvArgs dd_gemv_o(const dd_lm* h, int layer) {
  GemvArgs a = dd_gemv_matrix(h, dd_weight(h, layer, DD_M_O), h->xop_q);
  dd_gemv_resid_out(a, h, h->lw[layer].norm2, h->ssq_b);
  return a;
}
static inline GemvArgs dd_gemv_gate_up(const dd_lm* h, int layer) {
  GemvArgs a = dd_gemv_matrix(h, dd_weight(h, layer, DD_M_GATE_UP), h->xop_d);
  a.n_tiles /= 2;                                                   // EPI_SILU counts gate/up PAIRS
  dd_gemv_norm_in(a, h, h->ssq_b, h->d / 16);
  a.xop_next = h->xop_ff, a.S_next = h->S_ff;
  return a;
}
static inline GemvArgs dd_gemv_down(const dd_lm* h, int layer) {     // the norm that follows: the next layer's first, or the final one
  GemvArgs a = dd_gemv_matrix(h, dd_weight(h, layer, DD_M_DOWN), h->xop_ff);
  dd_gemv_resid_out(a, h, layer + 1 < h->Lyr ? h->lw[layer + 1].norm1 : h->final_norm, h->ssq_a);
  return a;
}
static inline GemvArgs dd_gemv_lm_head(const dd_lm* h, int ssq_n) {
  GemvArgs a = dd_gemv_matrix(h, dd_weight(h, 0, DD_M_LM_HEAD), h->xop_d);
  dd_gemv_norm_in(a, h, h->ssq_a, ssq_n);
  a.ldo = h->Vpad, a.n_valid = h->V;
  return a;
}

// -----------------------------------------------------------------------------------------------
// Prefill: the GemmArgs of the same five launches over M rows in the A planes a_hi / a_lo (the caller's scratch: the solo p1 / p2
// planes or the batch's pb planes).  The caller adds the destination (out, qbuf, kc / vc, o_hi / o_lo, pos0, the seq_* table)
// and points the launch at its matrix with dd_gemm_weight.
// -----------------------------------------------------------------------------------------------
static inline GemmArgs dd_gemm_rows(const dd_lm* h, const WMat& m, const uint16_t* a_hi, const uint16_t* a_lo, int M) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.wf = h->wf;
  g.a_hi = a_hi, g.a_lo = a_lo, g.M = M, g.S = m.S, g.n_tiles = m.n_tiles;
  return g;
}
static inline GemmArgs dd_gemm_qkv(const dd_lm* h, int layer, const uint16_t* a_hi, const uint16_t* a_lo, int M) {
  GemmArgs g = dd_gemm_rows(h, dd_weight(h, layer, DD_M_QKV), a_hi, a_lo, M);
  g.T_cap = h->T_cap, g.q_tiles = h->q_tiles, g.k_tiles = h->k_tiles, g.q_dim = h->q_dim, g.kv_dim = h->kv_dim, g.kv16 = h->kv16;
  g.rope_cos = h->rope_cos, g.rope_sin = h->rope_sin;
  return g;
}
static inline GemmArgs dd_gemm_o(const dd_lm* h, int layer, const uint16_t* a_hi, const uint16_t* a_lo, int M) {
  GemmArgs g = dd_gemm_rows(h, dd_weight(h, layer, DD_M_O), a_hi, a_lo, M);
  g.ldo = h->d;
  return g;
}
static inline GemmArgs dd_gemm_gate_up(const dd_lm* h, int layer, const uint16_t* a_hi, const uint16_t* a_lo, int M) {
  GemmArgs g = dd_gemm_rows(h, dd_weight(h, layer, DD_M_GATE_UP), a_hi, a_lo, M);
  g.ld_planes = h->dff;
  return g;
}
static inline GemmArgs dd_gemm_down(const dd_lm* h, int layer, const uint16_t* a_hi, const uint16_t* a_lo, int M) {
  GemmArgs g = dd_gemm_rows(h, dd_weight(h, layer, DD_M_DOWN), a_hi, a_lo, M);
  g.ldo = h->d;
  return g;
}
static inline GemmArgs dd_gemm_lm_head(const dd_lm* h, const uint16_t* a_hi, const uint16_t* a_lo, int M) {
  GemmArgs g = dd_gemm_rows(h, dd_weight(h, 0, DD_M_LM_HEAD), a_hi, a_lo, M);
  g.ldo = h->Vpad, g.n_valid = h->V;
  return g;
}
// g.W / g.wscale for matrix `which` of `layer`.  fp8 / MXFP4 storage: the GEMM runs on a bf16 expansion of ONE matrix at a time
// (exact) in h->deq_tmp, enqueued here; fp8 row scales go to the GEMM's epilogue, MXFP4 block scales are applied by the expansion.
static inline int dd_gemm_weight(const dd_lm* h, int layer, int which, GemmArgs& g, hipStream_t st) {
  const WMat m = dd_weight(h, layer, which);
  if (!h->wq) {
    g.W = m.W;
    return DD_OK;
  }
  g.W = h->deq_tmp;
  if (h->wq == DD_WQ_MXFP4) return ddk_dequant_tiles_mxfp4(m.W, (const uint32_t*)m.scale, h->deq_tmp, m.n_tiles, m.S, st);
  g.wscale = m.scale;
  return ddk_dequant_tiles(m.W, h->deq_tmp, m.n_tiles, m.S, st);
}
