// Internal launch interface between api.cpp and the .hip kernel files.  Every launcher only enqueues
// work on `stream` (no allocation, no synchronisation) and returns the hipError_t of the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pio {

enum OperandType { OP_F16 = 0, OP_BF16 = 1 };

// ---------------------------------------------------------------------------------------------
// ViT encoder
// ---------------------------------------------------------------------------------------------
enum GemmEpilogue {
  EPI_PATCH_EMBED = 0,  // x[b*Tp + G + p][n]  = acc + bias[n] + pos[(1+p)][n]          (fp32)
  EPI_QKV = 1,          // q/k [b][h][Tk][64], vT [b][h][64][Tk] (operand type) (+ fp32 qkv_last [B][T][3D])
  EPI_RESIDUAL = 2,     // x[m][n] += acc + bias[n], LayerScale folded into W and bias at load (fp32; the order of the sum: resid_join_ktile)
  EPI_GELU = 3,         // out16[m][n] = gelu_erf(acc + bias[n])                         (operand type)
  EPI_BIAS = 4          // out16[m][n] = acc + bias[n], row-major, no activation         (operand type): the V-only projection of a self-only block
};

#ifndef PIO_GEMM_WARM_NEXT      // extra workgroups that touch the next GEMM's weights (GemmArgs::pf); 0: never launched
#define PIO_GEMM_WARM_NEXT 1
#endif
struct GemmArgs {
  const void* A;   // [M][lda] operand type, K contiguous
  const void* W;   // [N][K]   operand type, K contiguous (torch Linear layout)
  const float* bias;
  int M, N, K, lda;
  // epilogue operands
  float* x;            // residual stream [B*Tp][D] fp32 (PATCH_EMBED, RESIDUAL)
  const float* pos;    // interpolated position table [1+n2][D] (PATCH_EMBED)
  void* out16;         // GELU / BIAS output [M][N]
  void* q; void* k; void* vT;   // QKV outputs
  float* qkv_last;     // optional fp32 capture [B][T][3D]
  int T, Tp, Tk, G, n2, D, H;  // tokens / padded rows per image / padded key count / global tokens / patches
  int act;             // EPI_GELU: 0 = exact-erf GELU (DINOv2), 1 = QuickGELU x * sigmoid(1.702 x) (OpenAI-CLIP towers)
  // optional: weights of the NEXT GEMM of the block, touched (one dword per 128-B line) by a few extra workgroups on compute units the
  // tiles leave idle, so that they wait in the Infinity Cache instead of HBM (round 4, vit_gemm.hip: "cold weights")
  const void* pf = nullptr;
  int pf_bytes = 0;
};
// the extra workgroups' body: workgroup e of ne, nthr threads each
__device__ __forceinline__ void gemm_warm_next(const GemmArgs& g, int e, int ne, int tid, int nthr) {
  const int lines = g.pf_bytes >> 7;
  const char* p = (const char*)g.pf;
  unsigned acc = 0;
  for (int l0 = e * nthr + tid; l0 < lines; l0 += 8 * ne * nthr) {       // eight loads in flight per lane
    unsigned r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int l = l0 + i * ne * nthr; r[i] = l < lines ? *(const unsigned*)(p + (size_t)l * 128) : 0u; }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc |= r[i];
  }
  asm volatile("" :: "v"(acc));
}

// EPI_RESIDUAL, the arithmetic EVERY GEMM kernel follows (one definition, so that an element of x never depends on the kernel, the
// launch size or the image's place in the launch that produced it).  LayerScale is folded into the operands at load (api.cpp:
// W' = op(ls[n] W[n][k]), b' = ls[n] b[n]), and
//     x_new[m][n] = ( sum over k ascending in MFMA steps of 16, from 0, with the OLD x[m][n] joining the sum after K-tile J(m, n) ) + b'[n]
// where a K-tile is 64 consecutive k and J(m, n) = min(e + 1, K / 64 - 1) with the class e = (m mod 4) + 4 ((n mod 256) / 128): the row's
// index mod 4 is the same wherever its image sits in a launch (images start at multiples of 8 rows: Tp % 8 == 0), the column half of the
// 256-grid always is -- a first version keyed the class to the row's place in the 256-row tile and an image's tokens changed bits
// with its position in the batch.  Why x joins in the MIDDLE of the sum: the persistent kernel (vit_gemm_roll.hip) fetches x one class
// per K-tile through 32 KiB of LDS while the multiplies run, so that the fp32 read of the residual stream costs no time of its own; at
// the end (or the start) of the sum all of a tile's x would be needed at once.  With the token on the accumulator REGISTER (32 x 32
// MFMA: register r of lane-half h holds row 8 (r >> 2) + 4 h + (r & 3)) a class is the registers r = c (mod 4) of EVERY lane, in the
// blocks of one column half.
__host__ __device__ constexpr int resid_class(int m, int n) { return (m & 3) + 4 * ((n >> 7) & 1); }
__host__ __device__ constexpr int resid_join_ktile(int e, int nk) { return e + 1 < nk - 1 ? e + 1 : nk - 1; }

hipError_t launch_vit_gemm(OperandType t, GemmEpilogue epi, const GemmArgs& a, hipStream_t s);
// The kernels launch_vit_gemm chooses between (values = PIO_GEMM_PATH_* of the C ABI's test hooks):  NARROW = k_vit_gemm with 64-row
// tiles (patch embed, proj / fc2), RES128 = its 128-row two-buffer residual form (lazy x join), WIDE128 = its 128-row form of qkv / fc1,
// K256 = k_vit_gemm256, ROLL = k_vit_gemm_roll.  EPI_BIAS is pinned to WIDE128 and K256 (route_vit_gemm); ROLL refuses it.  launch_vit_gemm == launch_vit_gemm_path(route_vit_gemm(epi, a)); route_vit_gemm is
// host only and returns -1 where no kernel takes the GEMM.  An explicit path launches only a kernel instantiated for the epilogue whose
// preconditions hold, else hipErrorInvalidValue (nothing launched).
enum GemmPath { GEMM_AUTO = 0, GEMM_NARROW = 1, GEMM_RES128 = 2, GEMM_WIDE128 = 3, GEMM_K256 = 4, GEMM_ROLL = 5 };
int route_vit_gemm(GemmEpilogue epi, const GemmArgs& a);
hipError_t launch_vit_gemm_path(OperandType t, GemmEpilogue epi, GemmPath p, const GemmArgs& a, hipStream_t s);
// 256 x 256 tiles, 8 waves (vit_gemm256.hip): same arithmetic per output element; launch_vit_gemm dispatches to it
bool vit_gemm256_fits(GemmEpilogue epi, const GemmArgs& a);
hipError_t launch_vit_gemm256(OperandType t, GemmEpilogue epi, const GemmArgs& a, hipStream_t s);
// persistent 256 x 256 workgroups with a rolling epilogue (vit_gemm_roll.hip): qkv without capture and fc1 at many tiles per CU, proj / fc2
// (EPI_RESIDUAL) from one tile per CU on
bool vit_gemm_roll_fits(GemmEpilogue epi, const GemmArgs& a);
hipError_t launch_vit_gemm_roll(OperandType t, GemmEpilogue epi, const GemmArgs& a, hipStream_t s);

struct VitAttnArgs {
  const void* q; const void* k; const void* vT;  // as written by EPI_QKV
  void* out;       // [B*Tp][D] operand type
  int B, H, T, Tp, Tk, D;
  float scale;     // head_dim^-0.5
  const int32_t* lens = nullptr;   // optional [B]: tokens of each sequence (keys >= lens[b] are masked); else T for all
  // optional query-row indirection (the sparse last block, api.cpp run_vit_block_rows): image b's queries are the rows
  // quads[i] + 0..3 (rows of the padded token matrix, b Tp + t) for i in [img_off[b], img_off[b + 1]), and query j of that list is
  // written to row 4 img_off[b] + j of `out` (compact rows).  Keys and values stay all T tokens of the image, in the same tile order;
  // a query is an MFMA column = one lane, so its bits do not depend on which tile or lane carries it.  max_rows = the longest
  // per-image list (4 x quads), which sizes the grid.
  const int32_t* quads = nullptr; const int32_t* img_off = nullptr; int max_rows = 0;
};
hipError_t launch_vit_attention(OperandType t, const VitAttnArgs& a, hipStream_t s);

// LayerNorm rows of x [M][D] fp32 -> operand type (out16) or fp32 (out32; compacts Tp -> T rows per image)
hipError_t launch_layernorm(OperandType t, const float* x, const float* w, const float* b, float eps, int M,
                            int D, void* out16, float* out32, int T, int Tp, hipStream_t s);
// ---- vit_fp32.hip: the exact-fp32 parity mode of the backbone (vit_operand_type = 2); plain kernels
hipError_t launch_im2col_f32(const float* imgs, int B, int S, int p, int n, int Kpad, float* out, hipStream_t s);
hipError_t launch_embed_scatter_f32(const float* emb, const float* pos, int B, int n2, int Tp, int G, int D, float* x, hipStream_t s);
hipError_t launch_attention_f32(const float* qkv, int B, int H, int T, int Tp, int D, float scale, const int32_t* lens, float* out, hipStream_t s);
hipError_t launch_resid_ls_f32(float* x, const float* y, const float* ls, size_t total, int D, hipStream_t s);
hipError_t launch_gelu_f32(float* y, size_t n, int act, hipStream_t s);
hipError_t launch_layernorm_f32(const float* x, const float* w, const float* b, float eps, int M, int D, float* y, hipStream_t s);
// ---- text_encoder.hip: the OpenAI-CLIP text tower (causal; caption s = rows [s Tp, s Tp + Tp), Tp = round_up(L, 8))
// x[s Tp + t] = tok[ids[s][t]] + pos[t] for t < L, zero rows t >= L; an id outside [0, V) gives a zero row and sets *err
hipError_t launch_text_embed(const int32_t* ids, int N, int L, int Tp, int V, int W, const float* tok, const float* pos, float* x,
                             int32_t* err, hipStream_t s);
// causal attention on MFMA, one workgroup per (caption, head): a.B = captions, a.T unused, round_up(a.Tp, 32) <= min(a.Tk, 128)
hipError_t launch_text_attention(OperandType t, const VitAttnArgs& a, hipStream_t s);
// the same in plain fp32 (parity mode): qkv [N*Tp][3D] -> out [N*Tp][D]
hipError_t launch_text_attention_f32(const float* qkv, int N, int H, int Tp, int D, float scale, float* out, hipStream_t s);
// out[s] = LayerNorm(x[s Tp + first argmax of ids[s]]) @ proj  (proj [W][E]; fp32)
hipError_t launch_text_pool(const float* x, const int32_t* ids, int N, int L, int Tp, int W, int E, const float* lw, const float* lb,
                            float eps, const float* proj, float* out, hipStream_t s);

// imgs [B][3][S][S] fp32 -> patch rows [B*n2][Kpad] (k = c*p*p + py*p + px; columns >= 3*p*p stay zero)
hipError_t launch_im2col(OperandType t, const float* imgs, int B, int S, int p, int n, int Kpad, void* out,
                         hipStream_t s);
// ---- alpha.hip: AlphaCLIP's region masks and four-channel patch rows
// masks out [R][grid][grid] u8: region r = union of boxes [box_off[r], box_off[r+1]) (xywh float32, floor-divided by `divisor`, end
// exclusive) and of the trace points [pt_off[r], pt_off[r+1]) (x, y float64 in [0, 1]); boxes / pts may be null when they hold none
hipError_t launch_region_masks(const float* boxes, const int32_t* box_off, const double* pts, const int32_t* pt_off, int R, int grid,
                               float divisor, uint8_t* out, hipStream_t s);
// rows [R*n2][Kpad] (type 0 fp16, 1 bf16, 2 fp32): columns [0, 3p^2) = image img_of_region[r] (null: r) as launch_im2col,
// [3p^2, 4p^2) = masks[r] (u8 [R][S][S], nonzero = 1; null: all ones); columns >= 4p^2 are not written
hipError_t launch_im2col_alpha(int type, const float* imgs, const int32_t* img_of_region, const uint8_t* masks, int R, int S, int p,
                               int n, int Kpad, void* out, hipStream_t s);
// x[b][0] = cls + pos[0]; x[b][1..R] = registers; x[b][T..Tp-1] = 0
// double-DINO boxes (P/src/bbox_utils.py:300-403): sequence s = (image, box) -> x[s] = [cls | registers | region patches]
// (final tokens; `slices` [Ns][4] = python-normalised ys, ye, xs, xe), zero rows up to Tp; lens[s] = its token count
hipError_t launch_box_sequences(const float* tokens, const int32_t* slices, int s_base, int Ns, int NB, int T, int Tp, int G,
                                int n, int D, int use_global, float* x, int32_t* lens, hipStream_t s);
// after the block: mode 0 = row 0 (cls), 1 = mean of rows [G_s, lens) (NaN for an empty region, like torch.mean)
hipError_t launch_box_seq_reduce(const float* x, const int32_t* lens, int Ns, int Tp, int D, int Gs, int mode, float* out,
                                 hipStream_t s);
hipError_t launch_token_init(float* x, const float* cls, const float* pos0, const float* reg, int B, int R, int T,
                             int Tp, int D, hipStream_t s);
// the sparse last block: xs[i] = x[quads[i >> 2] + (i & 3)] for the 4 nq compact rows (fp32 [.][D]), and row_map[b n2 + p] = i for
// every compact row that is patch p of image b (row_map [B][n2] int32; the caller has filled it with -1)
hipError_t launch_gather_rows(const float* x, const int32_t* quads, int nq, int T, int Tp, int G, int D, float* xs, int32_t* row_map,
                              hipStream_t s);
// The share of a launch's padded rows up to which the sparse last block runs (and its workspace is sized): 1 / kSparseShareDen.  Until
// the cut-over is measured it is one half; Engine.SPARSE_SHARE_DEN mirrors it.
static constexpr int kSparseShareDen = 2;

// ---- resnet.hip: RegionCLIP's CLIP ModifiedResNet tower (vit_arch 3); type 0 fp16, 1 bf16, 2 exact fp32 (the parity mode)
struct ConvArgs {
  const void* x;        // [B][H][W][Cin] (Cin padded to a multiple of 8; the padding channels are zero)
  const void* w;        // [Cout][ks][ks][Cin]
  const float* scale;   // [Cout] FrozenBN weight / sqrt(var + eps)
  const float* shift;   // [Cout] bias - mean * scale
  const void* res;      // [M][Cout] residual added after the BN (null: none)
  void* y;              // [B][Ho][Wo][Cout] (operand type)
  float* y32;           // out_f32: fp32 rows, see resnet.hip conv_store
  int B, H, W, Cin, Cout, ks, stride, pad, Ho, Wo;
  int relu;
  int out_f32, out_rows, out_off, valid;
};
// tile 0: route_conv's choice, 1: 64 x 64 workgroups, 2: 128 x 128 (the bits do not depend on it)
int route_conv(const ConvArgs& a);
hipError_t launch_conv(int type, const ConvArgs& a, int tile, hipStream_t s);
// imgs [B][3][S][S] fp32 -> [B][S][S][8] (channels 3..7 zero)
hipError_t launch_rn_input(int type, const float* imgs, int B, int S, void* out, hipStream_t s);
hipError_t launch_avgpool2(int type, const void* x, int B, int H, int W, int C, void* y, hipStream_t s);
// x [B][HW][C] -> out [B][Tp][C]: row 0 = mean over HW + pos[0], rows 1..HW = x + pos[1..], zero rows to Tp (pos fp32 [1 + HW][C])
hipError_t launch_attnpool_in(int type, const void* x, const float* pos, int B, int HW, int C, int Tp, void* out, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// attention read-out and region weighting (all fp32)
// ---------------------------------------------------------------------------------------------
// mean_logits [B][n2] = head-mean of (q_cls*scale).k_patch ; head_logits [B][Hr][n2] (may be null)
hipError_t launch_cls_logits(const float* qkv_last, int B, int T, int G, int D, int Hr, float scale,
                             float* mean_logits, float* head_logits, hipStream_t s);
hipError_t launch_softmax_rows(const float* in, float* out, int rows, int n, hipStream_t s);
hipError_t launch_trace_grids(const double* xy, const int32_t* offsets, int B, int n, float* grids, hipStream_t s);
// The largest grid the region kernels (k_region_reduce, k_bbox_weights, k_gaussian_map) hold: kRegionCellsPerThread cells per thread of a
// 256-thread workgroup, 1792 cells = a grid of 42 (the 40 x 40 patches of a ViT-B/16 at 640^2 included).  A thread adds its cells in
// index order, so a grid of at most 1536 cells gets the sums it got with 6 cells per thread, bit for bit: its 7th term is an exact + 0.
// kRegionLegacyCells: what they held before, and what every tower family but the plain CLIP ViT is still served up to (api.cpp,
// region_grid_ok).
static constexpr int kRegionCellsPerThread = 7;
static constexpr int kRegionMaxCells = 256 * kRegionCellsPerThread;
static constexpr int kRegionLegacyCells = 1536;
hipError_t launch_bbox_weights(const int32_t* boxes, int B, int NB, int n, int mode, float variance,
                               const int32_t* center_choice, float* attn, float* weights, int single_map,
                               float* single, hipStream_t s);
hipError_t launch_region_reduce(const float* tokens, int T, int G, int D, int n2, const float* weights,
                                const int32_t* img_index, int R, float scale, float* out, hipStream_t s);
// The same over COMPACT tokens [.][D] (the sparse last block): patch p of image i is row row_map[i n2 + p] (row_map [images][n2] int32;
// < 0: not computed -- such a patch must carry weight 0 and is skipped).  Same patches per wave, same order, same four-wave sum.
hipError_t launch_region_reduce_rows(const float* tokens, const int32_t* row_map, int D, int n2, const float* weights,
                                     const int32_t* img_index, int R, float scale, float* out, hipStream_t s);
hipError_t launch_ctx_clean(const float* dirty, const float* ctx, int R, int D, int rows_per_ctx, int mode, float alpha,
                            int normalize_inputs, float* out, hipStream_t s);
hipError_t launch_gaussian_map(int n, float variance, float* map, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// memory projection
// ---------------------------------------------------------------------------------------------
struct ProjectArgs {
  const float* bank;      // [M][D] raw rows
  const float* inv_norm;  // [M]
  int64_t M; int D;
  float* q;               // [N][D], normalised in place
  int N;
  float temperature;
  int normalize;
  float* out;             // [N][D]
  int n_best; float* best_sims;
  // workspaces (owned by the context)
  float* part_acc;        // [parts][N][D]
  float* part_ml;         // [parts][N][2]  (running max, running sum)
  float* part_best;       // [parts][N][n_best_cap]
  int parts; int n_best_cap;
  int part_rows = 0;      // rows of part_acc / part_ml the context allocated (16 parts; 24 parts allows the 48-query pass)
  float bank_scale;       // > 0 with bank_split: both GEMMs on split fp16 operands (bank * bank_scale = hi + lo; a power of two with
  const void* bank_split; // max|bank| * scale <= 2^15; [M][2][D] fp16, launch_split_bank); 0 / null: the exact fp32 form
};
hipError_t launch_mem_project(const ProjectArgs& a, hipStream_t s);
// one bank pass of launch_mem_project (k_project2 + k_project_combine) for the queries q0 .. q0 + 16 groups - 1 of a.q, which are unit
// rows already, on `parts` workgroups (1 .. 1024; part_acc / part_ml hold parts * 16 groups rows); a.parts / normalize / n_best unread
hipError_t launch_project_pass(const ProjectArgs& a, int groups, int q0, int parts, hipStream_t s);
// whether that pass runs the split-fp16 form on these operands (else exact fp32)
bool project_pass_is_split(const ProjectArgs& a, int groups);
// q normalised in place, then top-k cosine similarities and their rows per query (sims_scratch: [16][M] floats)
hipError_t launch_mem_topk(const float* bank, const float* inv_norm, int64_t M, int D, float* q, int N, int k, float* sims_scratch,
                           float* best_sims, int64_t* best_rows, hipStream_t s);
hipError_t launch_row_inv_norm(const float* bank, int64_t M, int D, float* inv_norm, hipStream_t s);
// out[0] = max |x[i]| as the bit pattern of a non-negative float (zeroed by the launcher); NaN / inf give >= 0x7F800000
hipError_t launch_abs_max(const float* x, int64_t n, uint32_t* out, hipStream_t s);
// out[row] = [fp16 hi of bank[row] * scale (D values) | fp16 lo (D values)]: the operand image of the split-fp16 projection
hipError_t launch_split_bank(const float* bank, int64_t M, int D, float scale, void* out, hipStream_t s);
hipError_t launch_revert(const float* x, const float* b, const float* A_pinv, int N, int D, int P, float* out,
                         hipStream_t s);

// ---------------------------------------------------------------------------------------------
// DeCap decoder (fp32, KV-cached greedy)
// ---------------------------------------------------------------------------------------------
// LayerNorm-folded linear layers (decoder.hip header): w = W * ln_w per input channel, c_j = sum_k w_jk,
// d_j = sum_k ln_b_k W_jk + b_j.
struct DecLayerW {
  const float *attn_w /*[3E][E] folded*/, *attn_c, *attn_d, *proj_w /*[E][E]*/, *proj_b;
  const float *fc_w /*[4E][E] folded*/, *fc_c, *fc_d, *fc2_w /*[E][4E]*/, *fc2_b;
  // the same matrices as split-fp16 operands (decoder.hip, k_dec_gemm_s; null: fp32 kernels only) and 1 / (their power-of-two scale x the
  // activations' scale)
  const void *attn_ws = nullptr, *fc_ws = nullptr, *fc2_ws = nullptr;
  float attn_un = 0.f, fc_un = 0.f, fc2_un = 0.f;
};
// W [n] fp32 -> split-fp16 layout ([row][8-k group][hi x 8 | lo' x 8]), same bytes; *unscale = 1 / (S x activation scale), S = the power of
// two that puts max |W| into [2^13, 2^14).  Synchronises (load time only).
hipError_t dec_split_weights(const float* W, size_t n, void* out, float* unscale, hipStream_t s);
static constexpr int DEC_MAX_PREFIXES = 256;       // rows of one greedy decode (ids only; log-probabilities: 64 per call)
static constexpr int DEC_SPLITK_COUNTERS = 128;    // arrival tickets / slab groups of the in-launch split-K (api.cpp allocates them)
static constexpr int DEC_TICKET_WORDS = DEC_SPLITK_COUNTERS + 2;   // ... + the LM head's arrival ticket and its tail's done-count (decoder.hip: k_lmhead_f16_fused<true>)
struct DecoderArgs {
  int N, steps, E, heads, layers, vocab, prefix_size;
  float eps;
  const float* prefix;        // [N][prefix_size]
  const float *clip_w /*[E][prefix]*/, *clip_b, *wte /*[V][E]*/, *wpe /*[P][E]*/;
  const float *head_w /*[V][E] = wte * ln_f.weight*/, *head_c, *head_d;
  const DecLayerW* layer;     // host array [layers]
  // workspaces
  float* x;      // [N][E] residual
  float* qkv;    // [N][3E]
  float* att;    // [N][E]
  float* hid;    // [N][4E]
  float* kcache; // [layers][N][max_steps][E]
  float* vcache;
  int max_steps;
  float* splitk_ws;       // [64 column groups][4 k-slices][4 row groups][256] partial tiles
  unsigned* splitk_cnt;   // [DEC_TICKET_WORDS] arrival tickets (zero between launches)
  int lm_tail;            // <= 16 prefixes: k_dec_select_filter as the ticketed tail of the LM head kernel (off by default: measured slower)
  float* logits; // [ceil(V/16)][N][4] per-workgroup (max, arg-max, sum-exp) partials of the LM head, or the
                 // approximate logits [N][round_up(V, 64)] of the fp16 filter
  // fp16 filter of the LM head (null head_w16: exact head only)
  const uint16_t* head_w16 = nullptr;   // [V][E] fp16 bits of head_w * 2^s
  float head_w16_unscale = 1.f;         // 2^-s
  float head_bound_coef = 0.f;          // 1.25e-3 * max_v |head_w[v]|_2
  void* xh = nullptr;                   // [N][E] fp16 copy of x (scaled per row)
  float* lm_stats = nullptr;            // [N][4] mu, rstd, 2^e, error bound
  float* lm_gmax = nullptr;             // [N][round_up(ceil(V/16), 64)] maxima of the approximate logits per 16 columns
  int32_t* ids;      // [N][steps]
  float* logprob;    // [N][steps] or null
  int pos_base = 0;  // position of the input that produces ids[.][0] (0: the DeCap prefix; P - 1 after a P-position prompt)
  // optional workspace of the batched prompt prefill (launch_decode_prompted): pre_rows rows of x / qkv / att / hid; null: position by position
  float *pre_x = nullptr, *pre_qkv = nullptr, *pre_att = nullptr, *pre_hid = nullptr;
  int pre_rows = 0;
};
hipError_t launch_decode_greedy(const DecoderArgs& a, hipStream_t s);
// The kernel-by-kernel tests' entry points (decoder.hip, end of file; test_hooks.cpp): the layer pass's own GEMM dispatch (selector: a line of the
// table above dec_layers, 0 family A, 1 family B, 2 by rows, 3 by rows with split-fp16 weights; epi 0 store + LN, 1 residual, 2 GELU + LN, 3 prefix
// projection) and its attention launches (form 0 step, 1 prefill, 2 ragged step, 3 ragged step through tab, 4 / 5 masked prefill passes).
hipError_t dec_test_layer_gemm(int selector, int epi, const float* W, const float* X, int rows, int Nout, int K, const float* bias, float* out,
                               const float* extra, const float* cvec, float eps, float* ws, unsigned* cnt, const void* Wsplit, float unscale,
                               hipStream_t s);
hipError_t dec_test_attention(int form, const float* qkv, float* kc, float* vc, float* att, int E, int heads, int N, int max_steps, int pos, int P,
                              const int32_t* plen, int split, const int32_t* tab, int tstride, hipStream_t s);
size_t dec_splitk_ws_floats();
// k_beam_step once for N images on caller-owned state, and the full-vocabulary head (lm_head_rows: kind 0 k_lm_logits_full, 1 k_lm_logits_rows;
// E = 768) on caller-owned rows and folded operands
hipError_t dec_test_beam_step(const float* lp, int N, int W, int V, int step, int eos0, int eos1, const int32_t* prow, float* scores, float* lens,
                              int32_t* stopped, int32_t* tok, int32_t* hist, int steps, int32_t* tab, int tstride, const float* wte,
                              const float* wpe, int npos, int E, float* x, hipStream_t s);
hipError_t dec_test_lm_head_rows(int kind, const float* head_w, const float* head_c, const float* head_d, float eps, const float* x, int rows,
                                 int V, bool log_softmax, float* stats, float* out, hipStream_t s);
// ViECap greedy search: prompt [N][P][E] at positions 0..P-1, then a.steps greedy tokens (a.pos_base = P - 1)
hipError_t launch_decode_prompted(const DecoderArgs& a, const float* prompt, int P, hipStream_t s);
// the same with a prompt length per prefix: prompt [N][Pmax][E] (k_build_prompt_ragged), plen [N] on the device (1 <= plen[n] <= Pmax <= 128,
// N <= 128); the batched prefill workspace is required (a.pre_x), the ticketed LM-head tail (a.lm_tail) is refused; a.pos_base is not read.
// split: prefixes with plen[n] <= split are prefilled on the GEMM family of a one-row-group prefill, the others on the tiled one (16; 256 when
// the uniform decode would take its prompt position by position) -- row n then has the ids of launch_decode_prompted on that row alone
hipError_t launch_decode_prompted_ragged(const DecoderArgs& a, const float* prompt, int Pmax, const int32_t* plen, int split, hipStream_t s);
// stop_at_eos: the two greedy decodes one segment of steps [s0, s1) at a time (0 <= s0 < s1 <= a.steps; a is the FULL decode's, a.steps
// included: it is the row stride of a.ids).  The segment at s0 == 0 starts with the decode's prologue (DeCap: the prefix projection; ViECap:
// the prompt prefill); the segments of [0, a.steps) in order issue exactly the launches of launch_decode_greedy / launch_decode_prompted.
hipError_t launch_decode_greedy_segment(const DecoderArgs& a, int s0, int s1, hipStream_t s);
hipError_t launch_decode_prompted_segment(const DecoderArgs& a, const float* prompt, int P, int s0, int s1, hipStream_t s);
// dec_stop.hip: first[n] = first column of ids [N][steps] in [s0, s1) with a stop id (stop1 < 0: one id) unless row n has one before s0
// (steps: none), *live = rows without one; only columns [s0, s1) are read.  out [N][steps] = ids with every column after first[n] set to
// ids[n][first[n]] (out != ids).  N <= DEC_MAX_PREFIXES, steps <= 64.
hipError_t launch_dec_stop_scan(const int32_t* ids, int N, int steps, int s0, int s1, int stop0, int stop1, int32_t* first, int32_t* live,
                                hipStream_t s);
hipError_t launch_dec_stop_pad(const int32_t* ids, const int32_t* first, int N, int steps, int32_t* out, hipStream_t s);
// teacher-forced pass over given tokens [N][Lmax] (rows of lens[n] tokens): nll[n] = sum over p + 1 < lens[n] of -log p(token p+1 | tokens <= p); N <= 64
hipError_t launch_lm_score(const DecoderArgs& a, const int32_t* tokens, const int32_t* lens, int Lmax, float* nll, hipStream_t s);
// beam search building blocks (N <= 16 beams per call; stats: [N][2] scratch; logp [N][V] = log softmax of the next-token logits)
hipError_t launch_lm_prefill(const DecoderArgs& a, const float* embeds, int P, float* stats, float* logp, hipStream_t s);
hipError_t launch_lm_advance(const DecoderArgs& a, const int32_t* tokens, const int32_t* src_rows, int pos, float* kscratch,
                             float* vscratch, float* stats, float* logp, hipStream_t s);
hipError_t launch_beam_select(const float* logp, const float* scores, const float* lens, const int32_t* stopped, int W, int V,
                              float* out_val, int64_t* out_idx, hipStream_t s);
// batched beam search: N images x W beams = a.N rows (<= 128, W <= 8), prompts embeds [N][Pmax][E] with plen [N] on the device (null: all
// Pmax), steps <= 64 selections; the batched prefill workspace is required (a.pre_x).  The state buffers are the handle's (beam_state).
// Per image and beam, in the order of the last selection: ids [N][W][steps] (-1 past the last selection), lens [N][W], scores / lens [N][W].
struct BeamArgs {
  const float* embeds;
  const int32_t* plen;
  int N, Pmax, W, steps, eos0, eos1;
  int npos;                   // rows of wpe
  int32_t *ids, *out_lens;
  float* out_scores;
  // state: stats [R][2], logp [R][V], prow / pimg / tok / stopped [R], scores / lens [R], tab [R][max_steps], hist [R][steps]
  float *stats, *logp, *scores, *lens;
  int32_t *prow, *pimg, *tok, *stopped, *tab, *hist;
};
hipError_t launch_lm_beam_search(const DecoderArgs& a, const BeamArgs& b, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// ClipCap head: nucleus sampling (sample.hip), the sampling decode loop and the MLP prefix mapper (decoder.hip)
// ---------------------------------------------------------------------------------------------
// One token per row of scores [N][ld] (V <= ld valid columns; raw logits or log-probabilities: a per-row constant is immaterial).
// Row n: inactive -> stop_id; NaN / inf anywhere -> stop_id; otherwise the top-p draw with uniform uniforms[n * u_stride] (sample.hip).
struct SampleArgs {
  const float* scores; int N, V, ld;
  float temperature, top_p;
  const float* uniforms; int u_stride;
  int stop_id;
  int32_t* active;            // [N] in / out
  int32_t* tokens; int tok_stride;
  int32_t* kept;              // [N] kept-set sizes, or null
};
hipError_t launch_nucleus_sample(const SampleArgs& a, hipStream_t s);
hipError_t launch_philox_uniforms(uint64_t seed, int N, int steps, float* u, hipStream_t s);     // u[n][k] = philox_uniform(seed, n, k)
hipError_t launch_sample_init(int N, int32_t* active, hipStream_t s);
hipError_t launch_sample_lens(const int32_t* ids, int N, int steps, int stop_id, int32_t* lens, hipStream_t s);
// prompt embeds [N][P][E] -> a.steps sampled tokens per row into a.ids [N][steps] (a.pos_base = P - 1; a.logits: [N][V] raw logits
// scratch; stats [N][2]); uniforms [N][steps] and active [N] on the device.  Every step runs; stopped rows emit stop_id.
hipError_t launch_lm_sample(const DecoderArgs& a, const float* prompt, int P, float temperature, float top_p, int stop_id,
                            const float* uniforms, int32_t* active, float* stats, int32_t* lens, hipStream_t s);
// ClipCap's MLP mapper: out [N][Nout] = tanh(x W1^T + b1) W2^T + b2 on the decode GEMM family; W1 [H][C], W2 [Nout][H] (nn.Linear
// layouts), H and Nout multiples of 768 / 16, C in {384, 512, 640, 768, 1024}; hid: [N][H] scratch, zeros: [Nout] zeros; N <= 128
hipError_t launch_clipcap_mapping(const float* x, int N, int C, int H, int Nout, const float* w1, const float* b1, const float* w2,
                                  const float* b2, const float* zeros, float* hid, float* out, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// ViECap head (viecap.hip): mapping network, entity logits, prompt assembly -- all fp32
// ---------------------------------------------------------------------------------------------
struct ViecapMapLayerW {
  const float *n1w, *n1b, *q_w /*[E][E]*/, *kv_w /*[2E][E]*/, *proj_w, *proj_b, *n2w, *n2b, *fc1_w /*[H][E]*/, *fc1_b, *fc2_w /*[E][H]*/, *fc2_b;
};
struct ViecapMapArgs {
  int N, C, E, Lp, Lc, heads, layers, hidden;
  float eps;
  const float* feats;        // [N][C], already L2-normalised
  const float *lin_w /*[Lp*E][C]*/, *lin_b, *prefix_const /*[Lc][E]*/;
  const ViecapMapLayerW* layer;
  float *lin, *x, *ln, *q, *kv, *att, *hid;   // workspaces: [N][Lp*E], [M][E] x 4, [M][2E], [M][H] with M = N (Lp + Lc)
  float* out;                // [N][Lc][E]
};
hipError_t launch_viecap_mapping(const ViecapMapArgs& a, hipStream_t s);
// C = alpha * A W^T (+ bias) (ReLU) (+= C): exact fp32, any M, N; K % 32 == 0
hipError_t launch_sgemm_tn(const float* A, int lda, const float* W, int ldw, const float* bias, float alpha, float* C, int ldc,
                           int M, int N, int K, int relu, int resid, hipStream_t s);
hipError_t launch_activation_f32(float* y, size_t n, int act, hipStream_t s);     // 2 tanh, 3 sigmoid, in place
hipError_t launch_build_prompt(const float* cont, const int32_t* tokens, const float* wte, int N, int Lc, int Lt, int E, int V,
                               int soft_first, float* prompt, hipStream_t s);
// hard prompt on the device (viecap.hip): top-k entities of probs [N][K] -> token rows [N][Lmax] padded per call (seg[n] = call of row n,
// NULL: one call) -> lens[n] = the call's longest row.  frag_off / frag_len [2K]: middle (2e) and last (2e + 1) fragment of entity e in frag_ids
struct ComposeArgs {
  const float* probs; int N, K;
  const int32_t *frag_ids, *frag_off, *frag_len;
  int head_off, head_len, empty_off, empty_len;
  int top_k; float threshold; int pad_id; const int32_t* seg; int Lmax;
  int32_t *tokens, *lens, *rawlen;                // rawlen [N]: scratch
};
hipError_t launch_compose_prompts(const ComposeArgs& a, hipStream_t s);
// prompt [N][Lc + Ltmax][E] with row n's hard prompt lt[n] tokens long (positions past Lc + lt[n]: zeros); plen[n] = Lc + lt[n]
hipError_t launch_build_prompt_ragged(const float* cont, const int32_t* tokens, const int32_t* lt, const float* wte, int N, int Lc, int Ltmax,
                                      int E, int V, int soft_first, float* prompt, int32_t* plen, hipStream_t s);
hipError_t launch_l2norm_rows(float* x, int N, int D, hipStream_t s);
// ---- preprocess.hip: image_transforms on the device (P/src/model.py:347-357; Pillow's 8-bit two-pass resampler) ----
struct PrepImage {
  int64_t src;                              // byte offset of the image's first pixel in `pixels` (RGB, HWC, row-major)
  int64_t tmp;                              // byte offset of its intermediate image [nr][nx][3] in `tmp`
  int32_t W, H;                             // source size
  int32_t x0, y0, nx, ny;                   // output window [y0, y0+ny) x [x0, x0+nx) that holds image content
  int32_t kh, kv;                           // taps per output column / row (strides of the coefficient tables)
  int32_t r0, nr;                           // first source row the vertical pass needs, number of such rows
  int32_t coef_h, coef_v, bnd_h, bnd_v;     // int32 offsets into `tables`: coefficients [n][k], bounds [n][2] = (min, count)
};
hipError_t launch_preprocess(const uint8_t* pixels, const PrepImage* imgs, const int32_t* tables, uint8_t* tmp,
                             const float* lut, int B, int S, int max_tmp_elems, float* out, hipStream_t s);


}  // namespace pio
