// Generation record (include/dropdec.h "Generation record"): one fixed-size record per emitted token, written by the step itself
// into a ring the caller attached, so that callers of the queued / graph-replayed decode forms can tell afterwards how sure the
// ensemble was about every token (reference: HF's `scores` behind chair_test/chair_test.py:341-346, masked_numbers of
// models/llava.py:661-662, the vote of models/llava.py:22-36, the winner's logits of models/llava.py:361-376).
//
// One launch per step, one 256-thread workgroup per sequence, two barriers.  It only reads what the step computed.
// Order of every reduction (part of the result: a sequence's record is the same bytes whichever launch shape or lane slot it has):
//   - thread t owns the column quads t, t + 256, t + 512, ... of a row (columns 4q .. 4q + 3) and visits its columns in ascending order;
//   - a wave combines its 64 lanes with the xor butterfly 32, 16, 8, 4, 2, 1 (commutative steps: every lane holds the same bits);
//   - the four waves' values are combined in wave order 0, 1, 2, 3.
// Top-8: every thread keeps the eight largest of ITS columns sorted in registers (fully unrolled insertion, static indices: no private
// scratch), a wave takes its eight largest from the lanes' list heads in eight shuffle rounds, the 32 candidates of the four waves are
// merged by wave 0.  Equal values: the lowest id first, the rule of k_row_epi_topk_lds (dd_dropout.hip).  Two passes over the rows in
// all (top-8 + un-masked maximum; sums + score row), each with four 16-byte loads per row in flight per thread.
#include <limits.h>

#include "dd_common.h"
#include "dd_engine_internal.h"

#define REC_THREADS 256
#define REC_WAVES (REC_THREADS / DD_WAVE)
#define REC_TOP 8
#define REC_UNROLL 4   // 16-byte loads in flight per thread and row
#define REC_LANES 8     // sequences per launch (pointer table by value, like k_step_end_lanes)

struct DDRecord {
  int32_t token, winner, votes, K, base_token;
  int32_t member_token[DD_MAX_MEMBERS];
  int32_t n_drop[DD_MAX_MEMBERS];
  float max, lse, logprob, entropy, base_logprob;
  int32_t top_id[REC_TOP];
  float top_logit[REC_TOP];
};
static_assert(sizeof(DDRecord) % 4 == 0 && sizeof(DDRecord) == 4 * (5 + 2 * DD_MAX_MEMBERS + 5 + 2 * REC_TOP), "DDRecord: 4-byte fields, no padding");

struct RecField {
  const char* name;
  int offset, count, is_float;
};
#define REC_F(f, n, fl) {#f, (int)offsetof(DDRecord, f), n, fl}
static const RecField g_rec_fields[] = {
    REC_F(token, 1, 0),        REC_F(winner, 1, 0),  REC_F(votes, 1, 0),   REC_F(K, 1, 0),       REC_F(base_token, 1, 0),
    REC_F(member_token, DD_MAX_MEMBERS, 0),          REC_F(n_drop, DD_MAX_MEMBERS, 0),           REC_F(max, 1, 1),
    REC_F(lse, 1, 1),          REC_F(logprob, 1, 1), REC_F(entropy, 1, 1), REC_F(base_logprob, 1, 1),
    REC_F(top_id, REC_TOP, 0), REC_F(top_logit, REC_TOP, 1)};

extern "C" size_t dd_record_bytes(void) { return sizeof(DDRecord); }
extern "C" int dd_record_field(int i, const char** name, int* offset, int* count, int* is_float) {
  const int n = (int)(sizeof(g_rec_fields) / sizeof(g_rec_fields[0]));
  DD_REQUIRE(i >= 0 && i < n, "dd_record_field: field %d of %d", i, n);
  if (name) *name = g_rec_fields[i].name;
  if (offset) *offset = g_rec_fields[i].offset;
  if (count) *count = g_rec_fields[i].count;
  if (is_float) *is_float = g_rec_fields[i].is_float;
  return DD_OK;
}

struct RecLanes {
  const DDState* st[REC_LANES];
  const float* rows[REC_LANES];        // the winner's row is rows + winner * Vpad (by_winner), else rows itself
  const float* base[REC_LANES];        // the un-masked pass' logits
  const int32_t* member_tok[REC_LANES];
  const int32_t* member_ids[REC_LANES];   // what the members voted with (hidden-state argmax for DD_VOTE_HIDDEN)
  const int32_t* n_drop[REC_LANES];
  const int32_t* argmax_base[REC_LANES];
  DDRecord* rec[REC_LANES];
  float* scores[REC_LANES];
  size_t scores_ld[REC_LANES];
  int cap[REC_LANES];
};

// (value, id) order of the top-k: larger value first, equal values: lower id first
__device__ __forceinline__ bool rec_better(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }
__device__ __forceinline__ void rec_wave_best(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (rec_better(ov, oi, v, i)) v = ov, i = oi;
  }
}

__global__ __launch_bounds__(REC_THREADS) void k_record_lanes(RecLanes t, int K, int V, int Vpad, int mode) {
  __shared__ float s_cv[REC_WAVES * REC_TOP];
  __shared__ int s_ci[REC_WAVES * REC_TOP];
  __shared__ float s_bmax[REC_WAVES];
  __shared__ float s_sum[REC_WAVES][3];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const DDState* st = t.st[q];
  int slot = 0;
  if (mode == DD_REC_STEP) {
    if (st->done) return;              // enqueued past an EOS: nothing is emitted, nothing is recorded
    slot = st->n_tok;
  }
  if (slot < 0 || slot >= t.cap[q]) return;     // the ring is full: never write past it
  const int win = K > 0 ? st->winner : -1;
  if (K > 0 && (win < 0 || win >= K)) return;
  const float* x = K > 0 ? t.rows[q] + (size_t)win * Vpad : t.rows[q];
  const float* xb = t.base[q];
  const int token = K > 0 ? t.member_tok[q][win] : t.argmax_base[q][0];
  DDRecord* r = t.rec[q] + slot;
  float* srow = t.scores[q] ? t.scores[q] + (size_t)slot * t.scores_ld[q] : nullptr;

  // Rows are read 16 bytes per lane, REC_UNROLL independent loads in flight per thread and row: one workgroup per sequence runs in
  // series with the step, so the launch is bound by load latency, not by bytes.  Thread t owns the column quads t, t + 256,
  // t + 512, ... and visits its columns in ascending order; rows are Vpad floats long (a multiple of 16, 16-byte aligned), columns
  // >= V are read and ignored.
  const f32x4_t* x4 = (const f32x4_t*)x;
  const f32x4_t* xb4 = (const f32x4_t*)xb;
  const int n4 = Vpad >> 2;

  // 1. one pass: every thread keeps the eight largest of its columns of the winner's row in registers (sorted, static indices only:
  //    no private scratch), and the maximum of its columns of the un-masked row
  float tv[REC_TOP];
  int ti[REC_TOP];
#pragma unroll
  for (int j = 0; j < REC_TOP; ++j) tv[j] = -INFINITY, ti[j] = INT_MAX;
  float mb = -INFINITY;
  for (int b0 = tid; b0 < n4; b0 += REC_THREADS * REC_UNROLL) {
    f32x4_t xv[REC_UNROLL], bv4[REC_UNROLL];
#pragma unroll
    for (int u = 0; u < REC_UNROLL; ++u) {
      const int idx = min(b0 + u * REC_THREADS, n4 - 1);    // every load is issued (no branch around a load); the mask is on the columns
      xv[u] = x4[idx], bv4[u] = xb4[idx];
    }
#pragma unroll
    for (int u = 0; u < REC_UNROLL; ++u) {
      const int idx = b0 + u * REC_THREADS;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = 4 * idx + c;
        if (idx < n4 && col < V) {
          const float v = xv[u][c];
          mb = fmaxf(mb, bv4[u][c]);
          if (v > tv[REC_TOP - 1]) {                        // strict: of equal values the earlier (lower) column stays ahead
            tv[REC_TOP - 1] = v, ti[REC_TOP - 1] = col;
#pragma unroll
            for (int j = REC_TOP - 1; j > 0; --j) {
              const bool up = tv[j] > tv[j - 1];
              const float fv = tv[j];
              const int fi = ti[j];
              tv[j] = up ? tv[j - 1] : fv, ti[j] = up ? ti[j - 1] : fi;
              tv[j - 1] = up ? fv : tv[j - 1], ti[j - 1] = up ? fi : ti[j - 1];
            }
          }
        }
      }
    }
  }
  // the wave's eight largest: eight rounds over the lanes' list heads; the lane whose head is taken moves its list up
  for (int p = 0; p < REC_TOP; ++p) {
    float bv = tv[0];
    int bi = ti[0];
    rec_wave_best(bv, bi);
    if (bi != INT_MAX && ti[0] == bi) {
#pragma unroll
      for (int j = 0; j + 1 < REC_TOP; ++j) tv[j] = tv[j + 1], ti[j] = ti[j + 1];
      tv[REC_TOP - 1] = -INFINITY, ti[REC_TOP - 1] = INT_MAX;
    }
    if (lane == 0) s_cv[wave * REC_TOP + p] = bv, s_ci[wave * REC_TOP + p] = bi;
  }
  mb = dd_wave_max(mb);
  if (lane == 0) s_bmax[wave] = mb;
  __syncthreads();
  float M = s_cv[0], Mb = s_bmax[0];
#pragma unroll
  for (int w = 1; w < REC_WAVES; ++w) M = fmaxf(M, s_cv[w * REC_TOP]), Mb = fmaxf(Mb, s_bmax[w]);

  // 2. sum exp(x - M), sum (x - M) exp(x - M), sum exp(xb - Mb); the score row
  float s = 0.f, a = 0.f, sb = 0.f;
  for (int b0 = tid; b0 < n4; b0 += REC_THREADS * REC_UNROLL) {
    f32x4_t xv[REC_UNROLL], bv4[REC_UNROLL];
#pragma unroll
    for (int u = 0; u < REC_UNROLL; ++u) {
      const int idx = min(b0 + u * REC_THREADS, n4 - 1);
      xv[u] = x4[idx], bv4[u] = xb4[idx];
    }
#pragma unroll
    for (int u = 0; u < REC_UNROLL; ++u) {
      const int idx = b0 + u * REC_THREADS;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = 4 * idx + c;
        if (idx < n4 && col < V) {
          const float v = xv[u][c];
          const float dx = v - M;
          const float e = expf(dx);
          s += e;
          a += e > 0.f ? e * dx : 0.f;                      // a column at -inf contributes p log p = 0, not 0 * -inf
          sb += expf(bv4[u][c] - Mb);
          if (srow) srow[col] = v;
        }
      }
    }
  }
  s = dd_wave_sum(s), a = dd_wave_sum(a), sb = dd_wave_sum(sb);
  if (lane == 0) s_sum[wave][0] = s, s_sum[wave][1] = a, s_sum[wave][2] = sb;
  __syncthreads();

  // 3. the record: wave 0 merges the candidates and writes the floats, wave 1 the members' columns
  if (wave == 0) {
    float cv = -INFINITY;
    int ci = INT_MAX;
    if (lane < REC_WAVES * REC_TOP) cv = s_cv[lane], ci = s_ci[lane];
    float sv = INFINITY;
    int si = -1;
    for (int p = 0; p < REC_TOP; ++p) {
      const bool after = cv < sv || (cv == sv && ci > si);
      float bv = after ? cv : -INFINITY;
      int bi = after ? ci : INT_MAX;
      rec_wave_best(bv, bi);
      if (lane == 0) r->top_id[p] = bi == INT_MAX ? -1 : bi, r->top_logit[p] = bv;   // fewer than eight columns: -1 / -inf
      sv = bv, si = bi;
    }
    if (lane == 0) {
      float S = s_sum[0][0], A = s_sum[0][1], Sb = s_sum[0][2];
#pragma unroll
      for (int w = 1; w < REC_WAVES; ++w) S += s_sum[w][0], A += s_sum[w][1], Sb += s_sum[w][2];
      const float logS = logf(S);
      const float lse = M + logS, lse_b = Mb + logf(Sb);
      const bool tok_ok = token >= 0 && token < V;
      int votes = 0;
      if (K > 0) {
        const int voted = st->voted;
        for (int k = 0; k < K; ++k) votes += t.member_ids[q][k] == voted ? 1 : 0;
      }
      r->token = token;
      r->winner = win;
      r->votes = votes;
      r->K = K;
      r->base_token = t.argmax_base[q][0];
      r->max = M;
      r->lse = lse;
      r->logprob = tok_ok ? x[token] - lse : -INFINITY;
      r->entropy = logS - A / S;
      r->base_logprob = tok_ok ? xb[token] - lse_b : -INFINITY;
    }
  } else if (wave == 1) {
    for (int k = lane; k < DD_MAX_MEMBERS; k += DD_WAVE) {
      r->member_token[k] = k < K ? t.member_ids[q][k] : -1;
      r->n_drop[k] = k < K ? t.n_drop[q][k] : 0;
    }
  }
}

int dd_record_launch(dd_lm* const* qs, int n, int K, int mode, hipStream_t st) {
  RecLanes t;
  int cnt = 0, V = 0, Vpad = 0;
  auto flush = [&]() -> int {
    if (!cnt) return DD_OK;
    k_record_lanes<<<cnt, REC_THREADS, 0, st>>>(t, K, V, Vpad, mode);
    DD_CHECK_LAUNCH();
    cnt = 0;
    return DD_OK;
  };
  DD_REQUIRE(K >= 0 && K <= DD_MAX_MEMBERS, "record: K=%d out of range", K);
  for (int m = 0; m < n; ++m) {
    dd_lm* q = qs[m];
    if (!q || !q->rec) continue;
    if (cnt && (q->V != V || q->Vpad != Vpad)) {
      int rc = flush();
      if (rc != DD_OK) return rc;
    }
    if (!cnt) memset(&t, 0, sizeof(t));
    V = q->V, Vpad = q->Vpad;
    t.st[cnt] = q->state;
    if (mode == DD_REC_FIRST) t.rows[cnt] = q->last_logits, t.base[cnt] = q->last_logits;
    else if (mode == DD_REC_FIRST_ENSEMBLE) t.rows[cnt] = q->member_logits, t.base[cnt] = q->image_logits + (size_t)q->L * q->Vpad;
    else t.rows[cnt] = K > 0 ? q->member_logits : q->base_logits, t.base[cnt] = q->base_logits;
    t.member_tok[cnt] = q->member_tok;
    t.member_ids[cnt] = q->cfg.vote_on == DD_VOTE_HIDDEN ? q->member_vote : q->member_tok;
    t.n_drop[cnt] = q->n_drop, t.argmax_base[cnt] = q->argmax_base;
    t.rec[cnt] = (DDRecord*)q->rec, t.scores[cnt] = q->rec_scores, t.scores_ld[cnt] = q->rec_scores_ld, t.cap[cnt] = q->rec_cap;
    if (++cnt == REC_LANES) {
      int rc = flush();
      if (rc != DD_OK) return rc;
    }
  }
  return flush();
}

extern "C" int dd_lm_set_record(dd_lm* h, void* rec_dev, int capacity, float* scores_dev, size_t scores_ld, void* stream) {
  (void)stream;
  DD_REQUIRE(h, "dd_lm_set_record: null handle");
  DD_REQUIRE(h->tp_world == 1, "dd_lm_set_record: this handle is a tensor-parallel shard: generation records are not available there "
                               "(include/dropdec.h \"Generation record\")");
  if (rec_dev) {
    DD_REQUIRE(capacity >= 1, "dd_lm_set_record: capacity %d (at least one record)", capacity);
    DD_REQUIRE(((uintptr_t)rec_dev & 3) == 0 && ((uintptr_t)scores_dev & 3) == 0, "dd_lm_set_record: buffers must be 4-byte aligned");
    DD_REQUIRE(!scores_dev || scores_ld >= (size_t)h->V, "dd_lm_set_record: scores_ld %zu is shorter than a row of V = %d logits", scores_ld, h->V);
  }
  const bool was = h->rec != nullptr, is = rec_dev != nullptr;
  if (was != is || (is && (h->rec != rec_dev || h->rec_cap != capacity || h->rec_scores != scores_dev || h->rec_scores_ld != scores_ld)))
    dd_engine_bump_epoch();            // graphs hold the launch and its pointers: captured steps of the other kind are not replayed
  h->rec = rec_dev;
  h->rec_cap = is ? capacity : 0;
  h->rec_scores = is ? scores_dev : nullptr;
  h->rec_scores_ld = is ? scores_ld : 0;
  return DD_OK;
}
