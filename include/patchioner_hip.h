/*
 * patchioner_hip.h -- C ABI of libpatchioner_hip.so, the MI355X (gfx950) implementation of the
 * Patch-ioner captioning hot path.
 *
 * The reference (Ruggero1912/Patch-ioner) is pure Python on PyTorch: it has no FFI.  Each entry point
 * below therefore replaces a *Python* function (or an inline block of Patchioner.forward) and cites
 * it as P/<file>:<lines> with P = /root/reference/Patch-ioner.  The reference-side binding a
 * maintainer would add is the ctypes stub shown in INTEGRATION.md (and shipped as
 * patchioner_amd/_lib.py).
 *
 * Conventions
 *   - plain C: pointers and sizes only, no torch / HIP types (streams travel as void*).
 *   - every function returns 0 on success or a negative pio_status; pio_last_error() gives the
 *     message of the last failure on the calling thread.
 *   - "dev" pointers are HIP device pointers owned by the caller; the library never frees them.
 *     Weights, the memory bank copy and all workspaces are owned by the handle (allocated in
 *     pio_create / pio_finalize_weights / pio_set_memory_bank; no allocation on the forward path).
 *   - one handle per (process, GPU); calls on one handle are serialised by the caller; all work of a
 *     call is enqueued on the given stream and nothing synchronises the device unless stated.
 *   - all floating-point tensors crossing the ABI are fp32, row-major, contiguous.
 */
#ifndef PATCHIONER_HIP_H
#define PATCHIONER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pio_context* pio_handle;
typedef void* pio_stream; /* hipStream_t */

typedef enum {
  PIO_OK = 0,
  PIO_ERR_INVALID_ARG = -1,
  PIO_ERR_HIP = -2,           /* a HIP runtime call failed (message has the HIP error string) */
  PIO_ERR_NOT_READY = -3,     /* weights / bank not loaded yet */
  PIO_ERR_UNKNOWN_WEIGHT = -4,
  PIO_ERR_SHAPE = -5,
  PIO_ERR_CAPACITY = -6       /* batch / prefix count above what pio_create sized */
} pio_status;

/* Static model description; mirrors what Patchioner.__init__ derives from the YAML config
 * (P/src/model.py:196-198, 285-286, 323-337) and decoder_config.pkl (P/src/decap/decap.py:66-71). */
typedef struct {
  /* ViT backbone (DINOv2 with registers) */
  int32_t embed_dim;          /* 384 / 768 / 1024 */
  int32_t depth;              /* 12 / 24 */
  int32_t num_heads;          /* backbone heads (12 for ViT-B) */
  int32_t patch_size;         /* 14 */
  int32_t num_registers;      /* 4 for *_reg models, else 0 */
  int32_t pretrain_grid;      /* 37: side of the learned position grid */
  int32_t crop_dim;           /* input side in pixels; must be a multiple of patch_size */
  float   vit_ln_eps;         /* 1e-6 */
  /* CLS-attention read-out quirk: 16 heads and scale 0.125 whatever the backbone (model.py:336-337) */
  int32_t readout_heads;
  float   readout_scale;
  /* DeCap decoder (GPT-2) */
  int32_t dec_layers;         /* 4 */
  int32_t dec_heads;          /* 4 */
  int32_t dec_embd;           /* 768 */
  int32_t dec_vocab;          /* 50257 */
  int32_t dec_positions;      /* 1024 */
  int32_t prefix_size;        /* clip_project input width (768, or 512 with the Talk2DINO inversion) */
  float   dec_ln_eps;         /* 1e-5 */
  /* capacities */
  int32_t max_batch;          /* images per pio_vit_forward call */
  int32_t max_prefixes;       /* prefixes per pio_decode_greedy / pio_mem_project call, <= 256 (log-probabilities: 64 rows per call) */
  int32_t max_steps;          /* decode steps (reference: 30) */
  /* numerics of the ViT MFMA path: 0 = fp16 operands, 1 = bf16 operands (fp32 accumulate either way); 2 = exact fp32
   * operands on the fp32 MFMA, a PARITY mode (plain kernels, ~20x slower) in which the whole path is held to the fp32
   * reference with no near-tie clause (csrc/vit_fp32.hip) */
  int32_t vit_operand_type;
  int32_t device;             /* HIP device ordinal */
  /* backbone family.  0: DINOv2 (torch.hub, P/src/model.py:342-343: LayerScale, exact-erf GELU, registers, interpolated
   * position grid).  1: the OpenAI-CLIP ViT the reference loads through timm with QuickGELU for its "DeCap original"
   * configurations (P/src/model.py:358-392, 786-796; configs/decap_B16*.k.yaml, decap_B32.k.yaml): patch 16 / 32, no
   * registers, norm_pre after the position add, no LayerScale, x * sigmoid(1.702 x), final norm on every token and the
   * bias-free head (embed_dim -> vit_out_dim) applied to every token; no qkv hook (has_attention = False, :864-865).
   * 2: AlphaCLIP's ViT (P/src/alphaclip/alpha_clip/model.py:351-380): arch 1 with a fourth, alpha input channel -- conv1(x) +
   * conv1_alpha(alpha) before the position add (weight key patch_embed.alpha.weight [D,1,p,p]); pio_vit_forward is the all-ones
   * alpha, pio_vit_forward_regions takes a mask per sequence.
   * 3: RegionCLIP's CLIP ModifiedResNet (P/src/regionclip/clip_backbone.py:112-300, forward_return_spatial_feats with 'res5'):
   * embed_dim = the attnpool width (32 rn_width), num_heads = embed_dim / 64, patch_size 32, crop_dim a multiple of 32; no
   * registers, no qkv hook; pio_vit_forward returns [B, 1 + (crop/32)^2, vit_out_dim] L2-normalised attnpool rows.  Weight keys
   * "rn.*" (weights.regionclip_to_engine: FrozenBN as scale / shift, q|k|v concatenated); depth, pretrain_grid, vit_ln_eps unused. */
  int32_t vit_arch;
  int32_t vit_out_dim;        /* width of the tokens pio_vit_forward returns: 0 = embed_dim; 512 for the CLIP ViT-B head */
  /* vit_arch 3 only (zero otherwise) */
  int32_t rn_layers[4];       /* Bottleneck units per stage: (3, 4, 6, 3) RN50, (4, 6, 10, 6) RN50x4 */
  int32_t rn_width;           /* stem width: 64 RN50, 80 RN50x4 */
  int32_t rn_attnpool_spatial; /* 1: patch rows = attnpool rows 1.. (use_attnpool_for_spatial_feats); 0: c_proj(x5) without attention */
  /* vit_arch 1 only (zero otherwise): the LAST vit_self_only_layers blocks attend to themselves only -- INViTE's extract_last_k_th_token
   * (P/src/INViTE/clipfolder/model.py:216-228: an attention mask that is -inf off the diagonal, so every softmax row is exactly 1 on
   * itself).  Such a block is x += proj(W_v ln_1(x) + b_v) followed by the MLP: the V third of in_proj is the only part of the fused
   * projection it multiplies, and no attention kernel runs.  0 <= value <= depth. */
  int32_t vit_self_only_layers;
} pio_config;

const char* pio_last_error(void);
const char* pio_version(void);

/* -- stream plumbing for pipeline.py (no reference counterpart: the reference runs on torch's current stream).
 *    A HIP stream restricted to the first `n_cus` compute units of `device` (hipExtStreamCreateWithCUMask), so that
 *    a latency-bound stage (the greedy decode) keeps compute units of its own beside the ViT GEMMs of the next
 *    batches.  n_cus <= 0 or >= the device's CU count: an ordinary stream.  `skip_cus` shifts the window. -- */
int pio_stream_create(int32_t device, int32_t skip_cus, int32_t n_cus, void** stream);
int pio_stream_destroy(void* stream);

/* -- a1: construction (replaces Patchioner.__init__ / from_config, P/src/model.py:98-662, 666-715) -- */
int pio_create(const pio_config* cfg, pio_handle* out);
int pio_destroy(pio_handle h);
/* A second decoder on the SAME weights (no reference counterpart; the reference decodes one batch at a time,
 * P/src/decap/decap.py:116-183): a handle that borrows `src`'s finalized decoder weights (read-only, not copied) and
 * owns its own activations, KV caches, scratch and decode graphs, so that pio_decode_greedy calls on `src` and on its
 * clones may run concurrently on different streams (pipeline.py decodes consecutive groups of prefixes that way).
 * Only pio_decode_greedy (and pio_destroy) are meaningful on a clone; `src` cannot be destroyed before its clones. */
int pio_clone_decoder(pio_handle src, pio_handle* out);

/* Upload one fp32 host tensor under its checkpoint key.  Keys are the reference checkpoints' own:
 *   backbone: "cls_token", "pos_embed", "register_tokens", "patch_embed.proj.weight", ...,
 *             "blocks.<i>.attn.qkv.weight", ..., "norm.bias"   (torch.hub dinov2 state_dict)
 *   decoder : "clip_project.model.0.weight|bias", "decoder.transformer.wte.weight", ...
 *             (DeCap checkpoint, P/src/decap/decap.py:61-79, 188-222)
 *   inversion: "talk2dino.A_pinv" [prefix_size, embed_dim], "talk2dino.b" [embed_dim]
 *             (P/src/model.py:618-627)
 * Unknown keys return PIO_ERR_UNKNOWN_WEIGHT (callers doing strict=False loading ignore it). */
int pio_load_weight(pio_handle h, const char* key, const float* host_data, const int64_t* shape, int32_t ndim);

/* Pack everything for the device: operand-precision copies, [out,in] transposes of the GPT-2 Conv1D
 * weights, bicubic-antialias interpolation of the position grid to crop_dim (DINOv2
 * interpolate_pos_encoding; cached per resolution).  Must be called once after the last pio_load_weight. */
int pio_finalize_weights(pio_handle h);

/* -- a9 state: the text memory bank (Im2TxtProjector.embs_dataset,
 *    P/src/decap/im2txtprojection/im2txtprojection.py:341-349).  Rows with zero norm are dropped as
 *    the reference does; inverse norms are precomputed once.  `rows_kept` may be NULL.
 *    Device memory: the fp32 copy (rows * dim * 4 B) and, unless vit_operand_type = 2 (the exact mode), a second image of the
 *    same size -- each row as the fp16 hi / lo halves of row * 2^k -- which is what pio_mem_project streams. */
int pio_set_memory_bank(pio_handle h, const float* host_bank, int64_t rows, int32_t dim, int64_t* rows_kept);

/* Same, from a device-resident fp32 bank (copied; no zero-row filtering -- the caller guarantees none). */
int pio_set_memory_bank_device(pio_handle h, const float* dev_bank, int64_t rows, int32_t dim);

/* -- a2 + a3: backbone forward with the last block's fused-QKV output captured
 *    (self.dino(imgs, is_training=True), P/src/model.py:782-783; hook P/src/dino_extraction.py:7-9).
 *    imgs_dev       [B,3,crop,crop]
 *    tokens_dev     [B,T,D]   final-LayerNorm'd tokens (cls | registers | patches), T = 1+R+n*n
 *    qkv_last_dev   [B,T,3D]  may be NULL */
int pio_vit_forward(pio_handle h, const float* imgs_dev, int32_t B, float* tokens_dev, float* qkv_last_dev,
                    pio_stream stream);

/* -- The same forward with a SPARSE last block, for callers that read only a few final tokens (trace regions: the region mean skips
 *    every patch whose grid weight is 0).  The last block's keys and values need every token, so everything up to its qkv projection
 *    runs on all rows; its query rows, attention output, proj, LayerNorm 2, fc1, fc2 and the final LayerNorm -- on the CLIP ViT also the
 *    head behind it -- run on the listed rows only.
 *    The unit is a quad: four consecutive rows of the padded token matrix [B * Tp] (Tp = T rounded up to 8) whose first row
 *    b * Tp + t is a multiple of 4.  quads_host [nq] = first rows, strictly ascending; img_off_host [B + 1] = offsets of every image's
 *    quads in that list, nq = img_off_host[B] (HOST memory, validated here and copied on `stream`: pinned memory must stay unchanged
 *    until the copy has run).  pio_host_trace_quads builds both from trace points.
 *    tokens_dev [4 * nq, Dout]: row 4 i + j = the final token of padded row quads[i] + j, bit-identical to pio_vit_forward's (Dout =
 *    vit_out_dim behind the CLIP head, else D).
 *    row_map_dev [B, n * n] int32: the compact row of every patch, -1 where it was not computed (pio_region_reduce_rows reads it).
 *    fp16 / bf16 DINOv2 towers and CLIP ViTs (vit_arch 1) without self-only blocks only; at most half of the launch's B * Tp rows may be listed (PIO_ERR_CAPACITY: call pio_vit_forward). */
int pio_vit_forward_rows(pio_handle h, const float* imgs_dev, int32_t B, const int32_t* quads_host, const int32_t* img_off_host,
                         float* tokens_dev, int32_t* row_map_dev, pio_stream stream);

/* -- AlphaCLIP (vit_arch 2): one tower pass per region, the alpha mask as the fourth input channel
 *    (forward_alphaclip_with_regions, P/src/model.py:1060-1354).  All pointers DEVICE.
 *    imgs_dev           [B,3,crop,crop] fp32, the call's images
 *    img_of_region_dev  [R] int32: sequence r reads image img_of_region[r] (NULL: image r)
 *    masks_dev          [R,crop,crop] u8, nonzero = 1 (NULL: all ones, = pio_vit_forward)
 *    tokens_dev         [R,T,vit_out_dim] as pio_vit_forward writes them;  1 <= R <= max_batch. */
int pio_vit_forward_regions(pio_handle h, const float* imgs_dev, const int32_t* img_of_region_dev, const uint8_t* masks_dev, int32_t R,
                            float* tokens_dev, pio_stream stream);

/* -- AlphaCLIP region masks (P/src/alphaclip/alpha_mask_utils.py): region r = the union of its boxes and trace points on a
 *    grid x grid raster, out masks_dev [R,grid,grid] u8 (0 / 1).  All pointers DEVICE.
 *    boxes_dev  [nb,4] float32 x, y, w, h; region r owns boxes [box_off[r], box_off[r+1]) (box_off_dev [R+1] int32).  Box rule of
 *               bbox_to_alpha_mask: end = x + w in float32, start and end floor-divided (torch's float //) by `divisor`, start
 *               clamped to [0, grid-1], end to [0, grid], end EXCLUSIVE, empty unless end > start on both axes.
 *    pts_dev    [np,2] float64 x, y; region r owns points [pt_off[r], pt_off[r+1]) (pt_off_dev [R+1] int32).  Point rule of
 *               map_traces_to_grid (P/src/bbox_utils.py:158-168), made binary.
 *    The tower's mask: grid = crop_dim, divisor 1; the patch average's: grid = crop_dim / patch_size, divisor patch_size.
 *    boxes_dev / pts_dev may be NULL when the table holds none. */
int pio_region_masks(pio_handle h, const float* boxes_dev, const int32_t* box_off_dev, const double* pts_dev, const int32_t* pt_off_dev,
                     int32_t R, int32_t grid, float divisor, uint8_t* masks_dev, pio_stream stream);

/* -- a4 + a5: CLS-row attention read-out and the two attention-weighted means
 *    (process_self_attention, P/src/dino_extraction.py:24-34; P/src/model.py:867-872).
 *    self_attn_dev [B,n*n]; head_maps_dev [B,H,n*n] (pre-softmax logits, may be NULL);
 *    avg_token_dev [B,D] (may be NULL); disentangled_dev [B,H,D] (may be NULL). */
int pio_cls_attention(pio_handle h, const float* qkv_last_dev, const float* tokens_dev, int32_t B,
                      float* self_attn_dev, float* head_maps_dev, float* avg_token_dev,
                      float* disentangled_dev, pio_stream stream);

/* -- a6: traces -> count grids (map_traces_to_grid, P/src/bbox_utils.py:158-168).
 *    xy_dev [P,2] float64 (x,y) of all points; offsets_dev [B+1] int32 CSR offsets; grids_dev [B,n,n]. */
int pio_trace_grids(pio_handle h, const double* xy_dev, const int32_t* offsets_dev, int32_t B,
                    int32_t total_points, float* grids_dev, pio_stream stream);

/* -- a7 weights: per-box weight maps (extract_bboxes_feats, P/src/bbox_utils.py:8-109).
 *    boxes_dev [B,NB,4] xywh already floor-divided by patch_size and truncated to int32;
 *    mode 0 uniform, 1 gaussian (variance > 0), 2 centre one-hot (variance == 0; `center_choice_dev`
 *    [B,NB,2] int32 gives the (y,x) picks for even spans, drawn by the host RNG like the reference's
 *    random.choice), 3 attention-map slice (attn_dev [B,n*n] is renormalised IN PLACE per box, in box
 *    order, as the reference does).
 *    weights_dev [B,NB,n*n]: zero outside the box; empty boxes give NaN rows like the reference's mean
 *    of an empty slice.  If single_map != 0 also produces the per-image normalised sum of maps
 *    (get_single_embedding_per_image) in single_dev [B,n*n], skipping boxes whose components sum < 0. */
int pio_bbox_weights(pio_handle h, const int32_t* boxes_dev, int32_t B, int32_t NB, int32_t mode, float variance,
                     const int32_t* center_choice_dev, float* attn_dev, float* weights_dev,
                     int32_t single_map, float* single_dev, pio_stream stream);

/* -- a6/a7/a8 reduction: out[r,:] = scale * sum_p weights[r,p] * patch_tokens[img[r], p, :]
 *    (P/src/model.py:1054; bbox_utils.py:53,79,109; model.py:90-92).
 *    tokens_dev [B,T,D] as written by pio_vit_forward (patch rows start at 1+R);
 *    weights_dev [R,n*n]; img_index_dev [R] int32 (NULL = row r uses image r); out_dev [R,D]. */
int pio_region_reduce(pio_handle h, const float* tokens_dev, int32_t B, const float* weights_dev,
                      const int32_t* img_index_dev, int32_t R, float scale, float* out_dev, pio_stream stream);

/* The same reduction over the COMPACT tokens of pio_vit_forward_rows: patch p of image i is row row_map_dev[i * n*n + p] of
 * tokens_dev (a patch without a row must carry weight 0).  row_map_dev points at the map of the first image the weights refer to.
 * Same patches per wave, same order of the sum: the result is pio_region_reduce's on the dense tokens, bit for bit. */
int pio_region_reduce_rows(pio_handle h, const float* tokens_dev, const int32_t* row_map_dev, const float* weights_dev,
                           const int32_t* img_index_dev, int32_t R, float scale, float* out_dev, pio_stream stream);

/* -- a8: fixed whole-image weight map (compute_region_means, P/src/model.py:45-94), variance > 0.
 *    map_dev [n*n]. variance >= 100 -> uniform. */
int pio_gaussian_map(pio_handle h, float variance, float* map_dev, pio_stream stream);

/* -- a9: memory projection (Im2TxtProjector.project, im2txtprojection.py:353-385), one pass over the bank
 *    with an online softmax.  q_dev [N,D] is L2-normalised IN PLACE (reference line 368).
 *    Arithmetic: operands as fp16 hi + lo pairs (22 significant bits), products on the fp16 matrix pipe, fp32
 *    accumulation, fp32 softmax: as close to an fp64 evaluation as an fp32 evaluation is; with
 *    vit_operand_type = 2 every product is an fp32 FMA in the reference's order.
 *    out_dev [N,D]; normalize != 0 L2-normalises the result; best_sims_dev [N,n_best] (may be NULL)
 *    receives the n_best largest cosine similarities in descending order. */
int pio_mem_project(pio_handle h, float* q_dev, int32_t N, float temperature, int32_t normalize,
                    float* out_dev, int32_t n_best, float* best_sims_dev, pio_stream stream);

/* Im2TxtProjector.project(..., return_argmax_text=True, return_n_best_sims=k) (P/src/decap/im2txtprojection/
 * im2txtprojection.py:367-375): q [N, D] is L2-normalised IN PLACE (line 368), then for every query the k largest cosine
 * similarities against the bank rows, descending (best_sims [N, k]), and the rows they belong to (best_rows [N, k], int64;
 * ties: the lower row, like torch.argmax; row indices count the rows KEPT at load, as the reference's do).  1 <= k <= 16. */
int pio_mem_topk(pio_handle h, float* q, int32_t N, int32_t k, float* best_sims, int64_t* best_rows, pio_stream stream);

/* -- f4 (bank build): ProjectionLayer.project_clip_txt (P/src/talk2dino/talk2dino.py:73-83), the step between CLIP's text
 *    features and the rows of the memory bank in Im2TxtProjector._build_support_memory (im2txtprojection.py:520-523):
 *    out = hidden_layer(act(linear_layer(x))) -- or linear_layer(x) alone when w2 is NULL (no hidden layer: the
 *    activation is then never applied, as in the reference's loop).  Exact fp32.  x [N, in_dim], w1 [out_dim, in_dim],
 *    w2 [out_dim, out_dim] (torch Linear layout), hidden = [N, out_dim] scratch (needed with w2), out [N, out_dim];
 *    act: 0 none, 1 relu, 2 tanh, 3 sigmoid (from_config's choices, :44-53); widths are multiples of 32. */
int pio_text_project(pio_handle h, const float* x, int32_t N, int32_t in_dim, const float* w1, const float* b1, int32_t out_dim,
                     const float* w2, const float* b2, int32_t act, float* hidden, float* out, pio_stream stream);

/* -- a10: (x - b) @ A_pinv^T (revert_transformation, P/src/embedding_utils.py:17-25). x_dev [N,D] ->
 *    out_dev [N,prefix_size]. */
int pio_revert_transformation(pio_handle h, const float* x_dev, int32_t N, float* out_dev, pio_stream stream);

/* -- a11 + a12: greedy decode (decoding_batched, P/src/decap/decap.py:116-155), KV-cached.
 *    prefix_dev [N,prefix_size]; ids_dev [N,steps] int32; logprob_dev [N,steps] per-token
 *    log-probabilities (may be NULL; the reference's score is exp of their row sum). */
int pio_decode_greedy(pio_handle h, const float* prefix_dev, int32_t N, int32_t steps, int32_t* ids_dev,
                      float* logprob_dev, pio_stream stream);

/* -- stop_at_eos, DeCap / CapDec: pio_decode_greedy that ends once every row has emitted `eos_id`.  The reference cuts each caption at its
 *    first end-of-text on the host (P/src/decap/decap.py:173, `.split('<|endoftext|>')[0]`), so nothing a row decodes after it is read.
 *    The decode runs in segments of `seg` steps (seg >= 1; seg >= steps: one segment), each the launches pio_decode_greedy issues for those
 *    steps; after a segment the count of rows without a stop goes to pinned host memory, the host waits on an event behind that copy
 *    (hipEventSynchronize) and launches the next segment only if a row is left.  BLOCKING by nature: for the synchronous paths only.
 *    ids_dev [N,steps] = canon(ids of pio_decode_greedy): row n up to and including its first eos_id column f_n, then ids[n][f_n] repeated;
 *    a row without eos_id unchanged -- whatever seg is and whether or not the decode ended early.  No log-probabilities.
 *    On return *steps_run_host (host memory) = steps the device was given (a multiple of seg, or steps) and all work is enqueued; ids_dev is
 *    valid once the stream is synchronised.  Checks and capacities as pio_decode_greedy.  Not bracketed by pio_profile_enable. */
int pio_decode_greedy_stop(pio_handle h, const float* prefix_dev, int32_t N, int32_t steps, int32_t eos_id, int32_t seg, int32_t* ids_dev,
                           int32_t* steps_run_host, pio_stream stream);

/* ---- ViECap head (P/src/model.py:1394-1398 -> P/src/viecap/entrypoint.py:98-153) -----------------------
 * Weights arrive through pio_load_weight under the checkpoint's own names: `mapping_network.*` (ClipCap.py:122-153) and
 * `gpt.transformer.*` (GPT2LMHeadModel; stored like DeCap's `decoder.transformer.*`).  pio_create: dec_layers = 12,
 * dec_heads = 12, max_steps >= continuous prompt + hard prompt + 63 (and >= the longest caption pio_lm_score is to score; <= 256). */
/* Entity vocabulary embeddings [K, C] (host; retrieval_categories.py:61-95 normalises them per call: done once here). */
int pio_viecap_set_entities(pio_handle h, const float* host_embeddings, int32_t K, int32_t C);
/* continuous_prompt_length of the loaded mapping network (rows of prefix_const), 0 without one */
int pio_viecap_prompt_length(pio_handle h);
/* VieCap.forward, first half (entrypoint.py:108-110): feats [N, C] L2-normalised IN PLACE, then
 * MappingNetwork.forward -> out [N, continuous_prompt_length, 768]. */
int pio_viecap_mapping(pio_handle h, float* feats, int32_t N, float* out, pio_stream stream);
/* image_text_simiarlity (retrieval_categories.py:61-95) on the already normalised feats: out [N, K] =
 * softmax(feats . entities^T / temperature). */
int pio_viecap_entity_logits(pio_handle h, const float* feats, int32_t N, float temperature, float* out, pio_stream stream);
/* VieCap.compute_perplexity (P/src/viecap/entrypoint.py:155-172): GPT2LMHeadModel(input_ids, labels = input_ids).loss per
 * caption, as a sum.  tokens [N, Lmax] int32 (row n holds lens[n] token ids, the rest is ignored), lens [N] int32, all on
 * the device; nll [N] receives sum_{p + 1 < lens[n]} -log p(token_{p+1} | token_0..p) (exact fp32 head), so that the
 * reference's loss is nll / (lens - 1) and its perplexity exp of that (lens = 1: 0 / 0, NaN, as in the reference).
 * 1 <= N <= min(max_prefixes, 64), Lmax <= max_steps. */
int pio_lm_score(pio_handle h, const int32_t* tokens, const int32_t* lens, int32_t N, int32_t Lmax, float* nll, pio_stream stream);

/* word_embed + torch.cat + greedy_search (entrypoint.py:126-150, search.py:108-191): cont [N, Lc, 768] soft prompt,
 * tokens [N, Lt] int32 hard-prompt ids already padded to one length (pad_sequence), soft_first as in the config; `steps`
 * greedy tokens (64 in the reference) with a KV cache, no attention mask, no early stop -> ids [N, steps] int32.
 * cont == NULL: only_hard_prompt (entrypoint.py:130-131) -- the prompt is the word embeddings of `tokens` alone (Lt >= 1). */
int pio_viecap_decode(pio_handle h, const float* cont, const int32_t* tokens, int32_t N, int32_t Lt, int32_t soft_first,
                      int32_t steps, int32_t* ids, pio_stream stream);
/* stop_at_eos, ViECap: pio_viecap_decode that ends once every row has emitted eos0 or eos1 (eos1 < 0: one stop id).  greedy_search cuts a
 * row at its first full stop (P/src/viecap/search.py:172-190; at one row it returns there, :160-163).  Segments, the hand-over of the live
 * count, canonical ids [N, steps], *steps_run_host and the blocking nature: as pio_decode_greedy_stop; checks as pio_viecap_decode.  The
 * segment graphs of up to 8 decode shapes (N, prompt length, steps, seg, stop ids) are kept, each captured as a decode first reaches it. */
int pio_viecap_decode_stop(pio_handle h, const float* cont, const int32_t* tokens, int32_t N, int32_t Lt, int32_t soft_first, int32_t steps,
                           int32_t eos0, int32_t eos1, int32_t seg, int32_t* ids, int32_t* steps_run_host, pio_stream stream);

/* The hard prompt on the device (the pipelined head): top_entities + compose_discrete_prompts + tokenisation + pad_sequence.
 * probs [N, K] = pio_viecap_entity_logits' output.  Entities are taken in torch.topk order (descending probability, equal values by the
 * lower index, NaN first) up to top_k (1..8), cut at the first probability < threshold.  The token row is the concatenation of fragments
 * of frag_ids: [head_off, +head_len) then, per chosen entity e, its middle fragment (frag_off / frag_len [2e]) or, for the last one, its
 * last fragment ([2e + 1]); no entity: [empty_off, +empty_len).  seg [N]: caption call of each row (NULL: one call); rows are padded with
 * pad_id to Lmax and lens[n] = the longest row of row n's call (what pad_sequence makes the reference feed the language model).
 * tokens [N, Lmax] int32, lens [N] int32, scratch [N] int32; all device memory, nothing waits for the device. */
int pio_viecap_compose_prompts(pio_handle h, const float* probs, int32_t N, int32_t K, const int32_t* frag_ids, const int32_t* frag_off,
                               const int32_t* frag_len, int32_t head_off, int32_t head_len, int32_t empty_off, int32_t empty_len,
                               int32_t top_k, float threshold, int32_t pad_id, const int32_t* seg, int32_t Lmax, int32_t* tokens,
                               int32_t* lens, int32_t* scratch, pio_stream stream);
/* pio_viecap_decode with a hard-prompt length per row: row n's prompt is cont[n] and tokens[n, :lens[n]] (lens on the device,
 * 0 <= lens[n] <= Ltmax), i.e. P_n = Lc + lens[n] positions; its ids equal those of pio_viecap_decode on that row alone with
 * Lt = lens[n].  The graph depends on (N, Lc + Ltmax, steps) only.  Works on decoder clones (pio_clone_decoder). */
int pio_viecap_decode_ragged(pio_handle h, const float* cont, const int32_t* tokens, const int32_t* lens, int32_t N, int32_t Ltmax,
                             int32_t soft_first, int32_t steps, int32_t* ids, pio_stream stream);

/* beam_search (P/src/viecap/search.py:193-285; VieCap.forward calls it per image when using_greedy_search is false,
 * entrypoint.py:143-148) as three device steps; the bookkeeping between them (token lists, lengths, stop flags) is the caller's.
 * The W beams of an image are the N rows of these calls and keep KV caches on the handle (the reference re-runs every beam's whole
 * sequence each step).  N <= min(16, max_prefixes); logp_dev [N, vocab] receives log(softmax(logits)) of the next token, evaluated
 * as the reference does (softmax, then log).
 *   pio_lm_prefill: embeds_dev [N, P, 768] (the prompt, repeated per beam) at positions 0..P-1.
 *   pio_lm_advance: beams re-ordered first -- row n continues the sequence of row src_rows_dev[n] (NULL: no re-ordering) -- then
 *     tokens_dev[n] (int32) is appended at position `pos` (= P + tokens generated so far - 1 ... the position of the new token).
 *   pio_beam_select: one selection.  scores_dev == NULL: the first one, the W largest of row 0.  Otherwise candidate (b, v) =
 *     stopped[b] ? (v == 0 ? scores[b] / lens[b] : -inf) : (scores[b] + logp[b][v]) / (lens[b] + 1); the W largest in descending
 *     order (ties: lower b * vocab + v first) -> out_val_dev [W] fp32, out_idx_dev [W] int64 flat indices. */
/* word_embed + torch.cat alone (entrypoint.py:126-135): prompt_dev [N, Lc + Lt, 768] as pio_viecap_decode assembles it
 * (cont_dev NULL: only_hard_prompt, Lc = 0); what beam search starts from. */
int pio_viecap_build_prompt(pio_handle h, const float* cont_dev, const int32_t* tokens_dev, int32_t N, int32_t Lt, int32_t soft_first,
                            float* prompt_dev, pio_stream stream);
int pio_lm_prefill(pio_handle h, const float* embeds_dev, int32_t N, int32_t P, float* logp_dev, pio_stream stream);
int pio_lm_advance(pio_handle h, const int32_t* tokens_dev, const int32_t* src_rows_dev, int32_t N, int32_t pos, float* logp_dev,
                   pio_stream stream);
int pio_beam_select(pio_handle h, const float* logp_dev, const float* scores_dev, const float* lens_dev, const int32_t* stopped_dev,
                    int32_t W, float* out_val_dev, int64_t* out_idx_dev, pio_stream stream);

/* Beam search of many images at once, enqueue-only and graph-captured: N images x W beams are the rows of one decode, every selection
 * and its bookkeeping run on the device, nothing waits for it.  Image n gets, bit for bit, what the three calls above and the host's
 * fp32 bookkeeping give for it alone (VieCapHead.beam_search): its prompt embeds_dev[n, :P_n] (P_n = plen_dev[n], device memory,
 * 1 <= P_n <= Pmax; plen_dev NULL: all Pmax) is prefilled once (the W beams share those keys / values), then `steps` selections
 * (64: the reference's max_len) with eos ids eos0 / eos1.  An image whose W beams have all stopped keeps its state (the reference's break).
 * Results per image and beam, in the order of the last selection: ids_dev [N, W, steps] int32 (the beam's tokens; read the first lens
 * of them; -1 past the image's last selection), lens_dev [N, W] int32, scores_dev [N, W] fp32 = accumulated score / length.
 * Bounds: 1 <= W <= 8 (PIO_ERR_INVALID_ARG), N * W <= min(max_prefixes, 128), 1 <= Pmax <= 128, 1 <= steps <= 64 and
 * Pmax + steps - 1 <= max_steps (PIO_ERR_CAPACITY).  The graph depends on (N, W, Pmax, steps); works on decoder clones.
 * pio_viecap_build_prompt_ragged lays the ViECap prompts out for it: prompt_dev [N, Lc + Ltmax, 768], row n = cont[n] and
 * tokens[n, :lens[n]] in soft_first order, zero past P_n; plen_dev [N] = Lc + lens[n] (pio_viecap_decode_ragged's layout). */
int pio_viecap_build_prompt_ragged(pio_handle h, const float* cont_dev, const int32_t* tokens_dev, const int32_t* lens_dev, int32_t N,
                                   int32_t Ltmax, int32_t soft_first, float* prompt_dev, int32_t* plen_dev, pio_stream stream);
int pio_lm_beam_search(pio_handle h, const float* embeds_dev, const int32_t* plen_dev, int32_t N, int32_t Pmax, int32_t W, int32_t steps,
                       int32_t eos0, int32_t eos1, int32_t* ids_dev, int32_t* lens_dev, float* scores_dev, pio_stream stream);

/* -- ClipCap head (P/src/clipcap/entrypoint.py): the MLP prefix mapper, top-p (nucleus) sampling, the sampling decode loop.
 * The checkpoint arrives through pio_load_weight under its own names: clip_project.model.0.* [H, C] and clip_project.model.2.*
 * [Lp * 768, H] (MLP: Linear, Tanh, Linear; C in {384, 512, 640, 768, 1024}, H a multiple of 768) and gpt.* as for the ViECap head.
 *   pio_clipcap_mapping: feats_dev [N, C] -> out_dev [N, Lp, 768]; normalize != 0: the rows are L2-normalised first, on a copy
 *     (feats_dev is not written).  N <= min(max_prefixes, 128).  pio_clipcap_prefix_length: Lp (0 without a mapper).
 *   pio_nucleus_sample: one token per row of scores_dev [N, V] fp32 (V = the handle's vocabulary; raw logits or log-probabilities,
 *     a per-row constant is immaterial).  p = softmax(scores / temperature) (temperature <= 0: 1); the kept set is the reference's
 *     shifted top-p mask -- the largest token always, token i iff the probability mass of the tokens ABOVE it is <= top_p; every token
 *     tied with the edge is kept -- and the token is the smallest kept id whose kept-mass prefix sum in ascending id order exceeds
 *     uniforms_dev[n] x (kept mass), uniforms in [0, 1).  active_dev [N] int32 in / out: a row whose flag is 0 emits stop_id and stays 0;
 *     a row that draws stop_id turns 0; a row with a NaN (or an inf) emits stop_id.  tokens_dev [N] int32; kept_dev [N] int32 or NULL:
 *     the kept-set sizes (0 for rows that did not sample).  The result of a row does not depend on where it sits in the launch.
 *   pio_lm_sample: embeds_dev [N, P, 768] prefilled once, then `steps` rounds of sample and advance, enqueue-only and graph-captured
 *     (keyed on N, P, steps, temperature, top_p, stop_id); every flag lives on the device and nothing waits for it; works on decoder
 *     clones.  uniforms_dev [N, steps] or NULL: then u[n][k] is Philox4x32-10 with key = seed and counter (n, k, 0, 0), first output
 *     word >> 8 times 2^-24 (pio_host_philox_uniform is the same function on the host).  ids_dev [N, steps] int32 (stop_id from a row's
 *     first stop on); lens_dev [N] int32 = index of the first stop token + 1, or steps.  All `steps` rounds run.
 *     A call counts its rows from 0: a caller that splits a batch over several calls and wants the ids of the unsplit batch passes
 *     uniforms_dev filled by pio_host_philox_uniforms(seed, first row of the call, ...).
 *     Bounds: N <= min(max_prefixes, 128), P + steps - 1 <= max_steps (PIO_ERR_CAPACITY); otherwise PIO_ERR_INVALID_ARG. */
int pio_clipcap_mapping(pio_handle h, const float* feats_dev, int32_t N, int32_t normalize, float* out_dev, pio_stream stream);
int pio_clipcap_prefix_length(pio_handle h);
int pio_nucleus_sample(pio_handle h, const float* scores_dev, int32_t N, float temperature, float top_p, const float* uniforms_dev,
                       int32_t stop_id, int32_t* active_dev, int32_t* tokens_dev, int32_t* kept_dev, pio_stream stream);
int pio_lm_sample(pio_handle h, const float* embeds_dev, int32_t N, int32_t P, int32_t steps, float temperature, float top_p,
                  int32_t stop_id, uint64_t seed, const float* uniforms_dev, int32_t* ids_dev, int32_t* lens_dev, pio_stream stream);

/* -- measurement: live HIP-event timing of the launches a call makes, on the stream they are launched on.
 *    While enabled every bracketed launch records a (start, stop) event pair; pio_profile_read waits for the
 *    recorded events of one class and returns the summed device time, the launch count and the ALGORITHMIC
 *    flops / bytes of those launches (no padding, no recompute). */
typedef enum {
  PIO_PROF_VIT_GEMM = 0,     /* k_vit_gemm: patch-embed, qkv, proj, fc1, fc2 (flops) */
  PIO_PROF_VIT_ATTN = 1,     /* k_vit_attention (flops) */
  PIO_PROF_VIT_LN = 2,       /* k_layernorm (bytes) */
  PIO_PROF_MEM_PROJECT = 3,  /* k_project + combine (bytes: one pass over the bank per 16 queries) */
  PIO_PROF_DECODE = 4        /* the whole greedy-decode graph (bytes: all fp32 weights once per step) */
} pio_profile_class;
int pio_profile_enable(pio_handle h, int32_t on);   /* also clears previous records */
int pio_profile_read(pio_handle h, int32_t cls, double* total_ms, int64_t* launches, double* flops, double* bytes);

/* -- f.2: extract_bboxes_feats_double_dino (P/src/bbox_utils.py:300-403, called at model.py:983-992): for every
 *    (image, box) re-run the LAST ViT block on [cls | registers | the box's region patches] of the final tokens
 *    (cls / registers only with use_cls) and return row 0 (return_type 0, "cls") or the mean of the region rows
 *    (1, "avg"; NaN for an empty region).  "gaussian_avg" of the reference weights the INPUT patches and does not
 *    need the block: the host mirror builds those weights and calls pio_region_reduce.
 *    tokens [B][T][D] fp32 (pio_vit_forward output); slices DEVICE int32 [B*NB][4] = (y_start, y_end, x_start, x_end)
 *    patch-grid slices after Python slice normalisation; out [B*NB][D].  Sequences run in chunks of max_batch. */
int pio_bbox_double_dino(pio_handle h, const float* tokens, const int32_t* slices, int32_t B, int32_t NB, int32_t use_cls,
                         int32_t return_type, float* out, pio_stream stream);

/* -- f.4: Patchioner.ctx_cleaner (P/src/model.py:1425-1436, used by forward(cleaning_type=...) at model.py:879-922):
 *    dirty [R][D], row r cleaned with context row r / rows_per_ctx of ctx; cleaning_type 0 = "orthogonal_projection"
 *    (dirty - alpha * (dirty . ctx / |ctx|^2) * ctx), 1 = "contrastive_mask" (dirty * (1 - ctx / (|ctx| + 1e-6))).
 *    normalize_inputs: both are L2-normalised first (the clean_after_projection=False branch, model.py:907-913).
 *    out may alias dirty.  D <= 1024. -- */
int pio_ctx_clean(pio_handle h, const float* dirty, const float* ctx, int32_t R, int32_t D, int32_t rows_per_ctx,
                  int32_t cleaning_type, float alpha, int32_t normalize_inputs, float* out, pio_stream stream);

/* -- a0: model.image_transforms / image_transforms_no_crop on the device (P/src/model.py:347-357):
 *    T.Resize(resize_dim, BICUBIC) -> T.CenterCrop(crop_dim) -> T.ToTensor() -> T.Normalize(ImageNet mean / std)
 *    (mode 0), or T.Resize((resize_dim, resize_dim), BICUBIC) -> ToTensor -> Normalize (mode 1; crop_dim ignored),
 *    for B RGB uint8 images of different sizes.  Bit-exact to the host pipeline: torchvision's size rules and
 *    Pillow's two-pass 22-bit fixed-point 8-bit resampler (coefficient tables built on the host per image).
 *    pixels      : DEVICE, the images packed back to back, each H x W x 3 row-major
 *    offsets     : HOST, B byte offsets into `pixels`;  wh : HOST, B x (width, height)
 *    out         : DEVICE fp32 [B][3][S][S], S = crop_dim (mode 0) or resize_dim (mode 1) -- what pio_vit_forward takes */
int pio_preprocess(pio_handle h, const void* pixels, const int64_t* offsets, const int32_t* wh, int32_t B,
                   int32_t resize_dim, int32_t crop_dim, int32_t mode, float* out, void* stream);

/* ---- CLIP text tower (clip.model.CLIP.encode_text; the memory-bank build P/src/decap/im2txtprojection/
 *      im2txtprojection.py:511-524, 650-657 and Patchioner's online_texts, :491-493).  A handle of its own: a text-only
 *      encoder needs no ViT, and pio_config is unchanged.
 *      Weights use the checkpoint's own names: token_embedding.weight [V,W], positional_embedding [ctx,W],
 *      transformer.resblocks.{i}.{ln_1,ln_2}.{weight,bias}, .attn.in_proj_weight [3W,W], .attn.in_proj_bias,
 *      .attn.out_proj.{weight,bias}, .mlp.c_fc.{weight,bias} [4W,W], .mlp.c_proj.{weight,bias} [W,4W],
 *      ln_final.{weight,bias}, text_projection [W,embed_dim].  Other keys are refused (PIO_ERR_UNKNOWN_WEIGHT).
 *      All workspaces are allocated by pio_text_finalize; pio_text_encode allocates nothing. */
typedef struct pio_text_context* pio_text_handle;
typedef struct {
  int32_t device;             /* HIP device ordinal */
  int32_t width;              /* 512 (ViT-B/16, B/32) or 768 (ViT-L/14) */
  int32_t layers;             /* 12 */
  int32_t heads;              /* width / 64 */
  int32_t context_length;     /* 77 (<= 120) */
  int32_t vocab_size;         /* 49408 */
  int32_t embed_dim;          /* width of text_projection's output (512 / 768) */
  int32_t max_texts;          /* captions per pio_text_encode call */
  int32_t operand_type;       /* 0 = fp16 MFMA operands (fp32 accumulate, fp32 residual stream); 2 = exact fp32 (parity mode) */
} pio_text_config;

int pio_text_create(const pio_text_config* cfg, pio_text_handle* out);
int pio_text_destroy(pio_text_handle h);
int pio_text_load_weight(pio_text_handle h, const char* key, const float* host, const int64_t* shape, int32_t ndim);
int pio_text_finalize(pio_text_handle h);
/* ids_dev [N,L] int32 on the device (clip.tokenize rows: SOT ... EOT, zero padded; L <= context_length, any L >= 1);
 * out_dev [N,embed_dim] fp32 = ln_final(x[n, argmax ids[n]]) @ text_projection.  A caption's row has the same bits whatever N
 * and L hold it.  Synchronises the stream at the end (to report an id outside the vocabulary: PIO_ERR_INVALID_ARG). */
int pio_text_encode(pio_text_handle h, const int32_t* ids_dev, int32_t N, int32_t L, float* out_dev, pio_stream stream);

/* Introspection used by the host mirror and the tests. */
int pio_num_tokens(pio_handle h);     /* T */
int pio_grid_side(pio_handle h);      /* n */
int64_t pio_bank_rows(pio_handle h);
/* The form pio_mem_project takes on the loaded bank: 1 split fp16 operands, 0 exact fp32 (the fp32 parity mode, PIO_PROJECT_EXACT, a
 * non-finite or vanishing max|bank|, or a row whose norm lies below sqrt(dim) 2^-26 max|bank|: the split pair's measured range); -1 no bank. */
int pio_bank_form(pio_handle h);

/* Host-only (no GPU needed): the load-time position-grid interpolation of pio_finalize_weights
 * (DINOv2 interpolate_pos_encoding: bicubic, antialias, offset 0).  pos [1+grid*grid, dim] -> out [1+n*n, dim]. */
int pio_host_interpolate_pos_embed(const float* pos, int32_t grid, int32_t dim, int32_t n, float* out);
/* the same for the hub models WITHOUT registers (num_registers = 0): bicubic without antialias on the scale factor
 * (n + offset) / grid, offset 0.1 (facebookresearch/dinov2 vision_transformer.py interpolate_pos_encoding, reached from
 * P/src/model.py:342-343, 783). */
int pio_host_interpolate_pos_embed_plain(const float* pos, int32_t grid, int32_t dim, int32_t n, double offset, float* out);

/* Host-only: the Pillow resampling table pio_preprocess builds for output samples [first, first + count) of an axis
 * resized from in_size to out_size (bicubic; Resample.c precompute_coeffs + normalize_coeffs_8bpc).  kk must hold
 * count * pio_host_pil_ksize(in_size, out_size) int32, bounds 2 * count (min, taps). */
int pio_host_pil_ksize(int32_t in_size, int32_t out_size);
int pio_host_pil_table(int32_t in_size, int32_t out_size, int32_t first, int32_t count, int32_t* kk, int32_t* bounds);
/* Host-only: the quads a batch of traces needs (pio_vit_forward_rows).  xy [P, 2] float64, offsets [B + 1] CSR, as pio_trace_grids takes
 * them but in HOST memory; n = grid side, G = 1 + registers, Tp = padded rows per image.  A quad is listed when one of its rows is a
 * patch whose cell holds a point, by the arithmetic of pio_trace_grids (double: the [0, 1] test, x / (1.0 / n), the clamp to n - 1).
 * quads [cap], img_off [B + 1].  Returns the number of quads (>= 0), or a negative error (bad sizes, more than cap). */
int pio_host_trace_quads(const double* xy, const int32_t* offsets, int32_t B, int32_t n, int32_t G, int32_t Tp, int32_t* quads,
                         int32_t cap, int32_t* img_off);
/* The sampler's counter-based generator on the host (no device): Philox4x32-10, out[4] from counter ctr[4] and the 64-bit key
 * (key_lo, key_hi); and the uniform pio_lm_sample draws for (row, step) under `seed` -- the fp32 value k / 2^24, written to *u. */
int pio_host_philox4x32(const uint32_t* ctr, uint32_t key_lo, uint32_t key_hi, uint32_t* out);
int pio_host_philox_uniform(uint64_t seed, uint32_t row, uint32_t step, float* u);
/* out[n * steps + k] = the uniform of (row0 + n, k) under `seed`, n < N, k < steps: what pio_lm_sample draws for a call whose first row
 * is row `row0` of a larger batch, for callers that split a batch over several calls and pass uniforms_dev. */
int pio_host_philox_uniforms(uint64_t seed, uint32_t row0, int32_t N, int32_t steps, float* out);
/* The loader's LayerNorm fold of a linear layer (HOST pointers): W [out][in] (in_major: [in][out], as GPT-2's Conv1D stores it), ln_w / ln_b
 * [in], bias [out] or NULL -> w [out][in] = W * ln_w, c [out] = row sums of w, d [out] = W ln_b + bias, so that
 * LN(x) W^T + bias = r (x w^T - mu c) + d.  The decoder kernel tests take their device operands from it. */
int pio_host_ln_fold(const float* W, int32_t in_major, int64_t in, int64_t out, const float* ln_w, const float* ln_b, const float* bias, float* w,
                     float* c, float* d);

/* ---- Test hooks: the ViT block kernels one at a time, for the kernel-by-kernel tests.  Caller-owned DEVICE pointers (torch
 *      tensors' data_ptr()), the current HIP device, no pio_handle.  Every size is validated before anything is launched; a refused
 *      call returns PIO_ERR_INVALID_ARG (or PIO_ERR_HIP with the HIP error) with pio_last_error() set and launches nothing.
 *      Buffer extents cannot be checked: they are the caller's (the shapes below). */
enum {
  PIO_GEMM_EPI_PATCH_EMBED = 0,  /* x[b*Tp + G + p][n] = acc + bias[n] + pos[1 + p][n]      (fp32; p = m mod n2, b = m / n2) */
  PIO_GEMM_EPI_QKV = 1,          /* q, k [B][H][Tk][64], vT [B][H][64][Tk] (operand type; rows m = b*Tp + t) (+ qkv_last [B][T][3D] fp32) */
  PIO_GEMM_EPI_RESIDUAL = 2,     /* x[m][n] = old x joined into the sum + bias[n]                 (fp32, in place) */
  PIO_GEMM_EPI_GELU = 3,         /* out16[m][n] = GELU(acc + bias[n]): act 0 exact erf, 1 QuickGELU (operand type) */
  PIO_GEMM_EPI_BIAS = 4          /* out16[m][n] = acc + bias[n], plain rows (operand type): pio_test_vit_vonly only (WIDE128 and K256) */
};
enum {
  PIO_GEMM_PATH_AUTO = 0,        /* what the forward passes take (the dispatch by tile count) */
  PIO_GEMM_PATH_NARROW = 1,      /* 128-wide kernel, 64-row tiles, three buffers: patch embed, residual */
  PIO_GEMM_PATH_RES128 = 2,      /* 128-wide kernel, 128-row tiles, two buffers, lazy x join: residual, K / 64 >= 10 */
  PIO_GEMM_PATH_WIDE128 = 3,     /* 128-wide kernel, 128-row tiles, one buffer: qkv, GELU */
  PIO_GEMM_PATH_K256 = 4,        /* 256 x 256 kernel: patch embed, qkv, GELU */
  PIO_GEMM_PATH_ROLL = 5         /* persistent rolling kernel: qkv without capture (Tp >= 256), GELU (Tp >= 256), residual (K / 64 >= 12) */
};
typedef struct {
  const void* A;          /* [M][lda] operand type */
  const void* W;          /* [N][K] operand type */
  const float* bias;      /* [N] */
  int32_t M, N, K, lda;
  float* x;               /* PATCH_EMBED: [B*Tp][D] (written); RESIDUAL: [M][N] (read and written) */
  const float* pos;       /* PATCH_EMBED: [1 + n2][D] */
  void* out16;            /* GELU: [M][N] */
  void* q; void* k; void* vT;
  float* qkv_last;        /* QKV: optional fp32 capture [B][T][3D] (NULL: none) */
  int32_t T, Tp, Tk, G, n2, D, H, act;
  const void* pf;         /* optional: bytes the extra cache-warming workgroups read (never written) */
  int32_t pf_bytes;
} pio_test_gemm_args;
/* operand 0 = fp16, 1 = bf16; *path_taken (may be NULL) = the PIO_GEMM_PATH_* that ran */
int pio_test_vit_gemm(int32_t operand, int32_t epi, int32_t path, const pio_test_gemm_args* args, int32_t* path_taken, pio_stream stream);
/* host only: the PIO_GEMM_PATH_* PIO_GEMM_PATH_AUTO takes for these sizes, PIO_ERR_INVALID_ARG where no kernel takes them */
int pio_test_gemm_route(int32_t epi, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t D, int32_t Tp, int32_t has_capture);
/* The V-only projection of a self-only block (pio_config.vit_self_only_layers) on its own: out16 [M][D] = A [M][D] . Wv^T + bv in the
 * operand type, where Wv / bv are rows [2D, 3D) of the FUSED in_proj the caller hands over (in_proj_w [3D][D] operand type, in_proj_b
 * [3D] fp32) -- the hook slices them as the engine does at load; the q and k thirds are never read.  path: PIO_GEMM_PATH_AUTO,
 * _WIDE128 or _K256 (the others have no such epilogue and are refused); D % 256 == 0. */
int pio_test_vit_vonly(int32_t operand, int32_t path, const void* A, const void* in_proj_w, const float* in_proj_b, void* out16, int32_t M,
                       int32_t D, int32_t* path_taken, pio_stream stream);
/* kind 0: the ViT flash attention (lens: optional DEVICE [B], 1 <= lens[b] <= T: keys >= lens[b] masked); kind 1: the text tower's
 * causal attention (keys <= query; T, lens unused).  q, k [B][H][Tk][64], vT [B][H][64][Tk] -> out [B*Tp][D], operand type. */
int pio_test_attention(int32_t kind, int32_t operand, const void* q, const void* k, const void* vT, void* out, int32_t B, int32_t H,
                       int32_t T, int32_t Tp, int32_t Tk, int32_t D, float scale, const int32_t* lens, pio_stream stream);
/* LayerNorm rows of x [M][D] fp32 (D % 4 == 0, D <= 1024): out16 [M][D] operand type, or (out16 NULL) out32 fp32 with the rows
 * t >= T of every Tp-row image dropped ([M / Tp * T][D]) */
int pio_test_layernorm(int32_t operand, const float* x, const float* w, const float* b, float eps, int32_t M, int32_t D, void* out16,
                       float* out32, int32_t T, int32_t Tp, pio_stream stream);
/* AlphaCLIP's four-channel patch rows (pio_vit_forward_regions' im2col): imgs [B][3][S][S] fp32, img_of_region [R] int32 (NULL: r),
 * masks [R][S][S] u8 (NULL: ones) -> out [R * (S/p)^2][Kpad] in operand type 0 fp16, 1 bf16, 2 fp32; columns >= 4 p^2 not written. */
int pio_test_im2col_alpha(int32_t operand, const float* imgs, const int32_t* img_of_region, const uint8_t* masks, int32_t R, int32_t S,
                          int32_t p, int32_t Kpad, void* out, pio_stream stream);

/* RegionCLIP tower kernels (vit_arch 3, csrc/resnet.hip), operand 0 fp16, 1 bf16, 2 exact fp32; all pointers DEVICE.
 * Convolution (replaces nn.Conv2d + FrozenBatchNorm2d [+ identity] + ReLU of Bottleneck.forward / ModifiedResNet.stem,
 * P/src/regionclip/clip_backbone.py:57-70, 237-245): x [B][H][W][Cin] NHWC, Cin % 8 == 0, w [Cout][ks][ks][Cin], ks 1 or 3 (pad
 * ks / 2), stride >= 1; y [B][Ho][Wo][Cout] operand type = relu?(rnd(rnd(rnd(conv) * scale + shift) + res)) with res [B][Ho][Wo][Cout]
 * or NULL; with y32 non-NULL (y NULL, res NULL) the same value before the residual, as fp32.  tile 0 = the forward's choice, 1 = 64 x
 * 64, 2 = 128 x 128 workgroups (ignored in fp32). */
int pio_test_conv(int32_t operand, const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y,
                  float* y32, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t relu,
                  int32_t tile, pio_stream stream);
/* nn.AvgPool2d(2) in NHWC: x [B][H][W][C] -> y [B][H/2][W/2][C] (clip_backbone.py:35, 55, 157) */
int pio_test_avgpool(int32_t operand, const void* x, int32_t B, int32_t H, int32_t W, int32_t C, void* y, pio_stream stream);
/* AttentionPool2d's input rows (clip_backbone.py:84-86): x [B][HW][C], pos [1 + HW][C] fp32 -> out [B][Tp][C]: row 0 = mean + pos[0],
 * rows 1..HW = x + pos[1..], zero rows to Tp */
int pio_test_attnpool_in(int32_t operand, const void* x, const float* pos, int32_t B, int32_t HW, int32_t C, int32_t Tp, void* out,
                         pio_stream stream);

/* k_nucleus_sample at any V, without a handle: pio_nucleus_sample's arguments with scores [N, V]. */
int pio_test_nucleus_sample(const float* scores, int32_t N, int32_t V, float temperature, float top_p, const float* uniforms, int32_t stop_id,
                            int32_t* active, int32_t* tokens, int32_t* kept, pio_stream stream);

/* Decoder kernels (csrc/decoder.hip) one launch at a time, through the layer pass's own dispatch.  E = 768 throughout.
 * pio_test_dec_workspace: the float count of the split-K workspace and the number of 32-bit ticket words a caller allocates (tickets zeroed). */
int pio_test_dec_workspace(int64_t* ws_floats, int32_t* ticket_words);
/* W [n] fp32 (n % 8 == 0, finite) -> the split-fp16 image (out: 4 n bytes) and *unscale (HOST pointer); synchronises the stream */
int pio_test_dec_split_weights(const float* W, int64_t n, void* out, float* unscale, pio_stream stream);
enum {
  PIO_DEC_GEMMS_FAMILY_A = 0,      /* k_dec_gemm, 4 waves x 12 chunks, per 128-row chunk (ragged step, beam step, ragged prefill pass 1) */
  PIO_DEC_GEMMS_FAMILY_B = 1,      /* k_dec_gemm_b per 128-row chunk (ragged prefill pass 2) */
  PIO_DEC_GEMMS_BY_ROWS = 2,       /* dec_gemm per 128-row chunk, no split weights (uniform batched prefill) */
  PIO_DEC_GEMMS_BY_ROWS_SPLIT = 3  /* dec_gemm on all rows, split-fp16 weights from 65 rows when given (uniform step) */
};
enum {
  PIO_DEC_EPI_STORE_LN = 0,        /* out = LN(x) W^T + b             Nout 2304, K 768   (W, bias = d, cvec: the loader's folded operands) */
  PIO_DEC_EPI_RESID = 1,           /* out += x W^T + b                Nout 768, K 768 or 3072 (3072: split-K, ws and tickets required) */
  PIO_DEC_EPI_GELU_LN = 2,         /* out = gelu_new(LN(x) W^T + b)   Nout 3072, K 768 */
  PIO_DEC_EPI_EMBED = 3            /* out = x W^T + b + extra         Nout 768, K 384 / 512 / 640 / 768 / 1024; selector ignored */
};
/* X [N][K], W [Nout][K], out [N][Nout], 1 <= N <= 256.  Wsplit (may be NULL): W's split-fp16 image, read by PIO_DEC_GEMMS_BY_ROWS_SPLIT only. */
int pio_test_dec_gemm(int32_t selector, int32_t epi, const float* W, const void* Wsplit, float unscale, const float* X, int32_t N, int32_t Nout,
                      int32_t K, const float* bias, const float* cvec, const float* extra, float eps, float* out, float* ws, uint32_t* tickets,
                      pio_stream stream);
enum {
  PIO_DEC_ATTN_STEP = 0,           /* every row at position pos */
  PIO_DEC_ATTN_PREFILL = 1,        /* rows [n][p], p < P: keys / values of all positions appended, then all positions attended */
  PIO_DEC_ATTN_RAGGED = 2,         /* row n at position plen[n] + pos */
  PIO_DEC_ATTN_RAGGED_TAB = 3,     /* ... history key / value j < position read from cache row tab[n * tstride + j] (clamped to [0, N)) */
  PIO_DEC_ATTN_MASK1 = 4,          /* prefill, appending only for rows with plen[n] <= split */
  PIO_DEC_ATTN_MASK2 = 5           /* prefill, appending only for rows with plen[n] > split */
};
/* qkv [rows][2304], att [rows][768] (rows = N, or N * P in the prefill forms), kcache / vcache [N][max_steps][768]; heads: 768 / heads a
 * multiple of 32, <= 256; max_steps <= 256.  plen / tab are DEVICE arrays; plen is copied back and checked (the stream is synchronised). */
int pio_test_dec_attention(int32_t form, const float* qkv, float* kcache, float* vcache, float* att, int32_t N, int32_t heads, int32_t max_steps,
                           int32_t pos, int32_t P, const int32_t* plen, int32_t split, const int32_t* tab, int32_t tstride, pio_stream stream);

/* Beam search kernels (csrc/decoder.hip) one launch at a time.
 * pio_test_beam_select: pio_beam_select (k_beam_select) with V the caller's: lp [W][V] (scores NULL: row 0 only), scores / lens [W] fp32,
 *   stopped [W] int32 -> out_val [W] fp32, out_idx [W] int64.  1 <= W <= 8, V >= W. */
int pio_test_beam_select(const float* lp, const float* scores, const float* lens, const int32_t* stopped, int32_t W, int32_t V, float* out_val,
                         int64_t* out_idx, pio_stream stream);
/* ONE k_beam_step launch (selection `step` of pio_lm_beam_search and the bookkeeping after it) for N images of W beams, rows r = n W + b,
 * all state the caller's and updated in place: lp [N W][V] (step 0: its first N rows, one per image), prow [N W] int32 (the prompt length
 * P_n, on every row of image n), scores / lens [N W] fp32, stopped / tok [N W] int32, hist [N W][steps] int32, tab [N W][tstride] int32,
 * wte [V][E], wpe [npos][E] -> x [N W][E] = wte[tok] + wpe[min(P_n + step, npos - 1)].  Refused before any launch: W outside 1..8, V < W,
 * steps outside 1..64, step outside 0..steps - 1, tstride outside 1..256, N outside 1..128, and any row with prow[r] < 1 or
 * prow[r] + step - 1 >= tstride (prow is copied back: the stream is synchronised). */
int pio_test_beam_step(const float* lp, int32_t N, int32_t W, int32_t V, int32_t step, int32_t eos0, int32_t eos1, const int32_t* prow, float* scores,
                       float* lens, int32_t* stopped, int32_t* tok, int32_t* hist, int32_t steps, int32_t* tab, int32_t tstride, const float* wte,
                       const float* wpe, int32_t npos, int32_t E, float* x, pio_stream stream);
/* The full-vocabulary head of the beam search and the sampler on caller-owned rows: k_row_stats, then kind 0 k_lm_logits_full (the per-image
 * path) or 1 k_lm_logits_rows (the batched path), then (log_softmax != 0) k_log_softmax_rows in place.  x [rows][768]; head_w [V][768],
 * head_c, head_d [V]: pio_host_ln_fold's w, c, d of the tied head (W = wte, LayerNorm ln_f, no bias); stats [rows][2] scratch (mean,
 * 1 / sqrt(var + eps)); out [rows][V].  1 <= rows <= 256. */
int pio_test_lm_head_rows(int32_t kind, const float* head_w, const float* head_c, const float* head_d, float eps, const float* x, int32_t rows,
                          int32_t V, int32_t log_softmax, float* stats, float* out, pio_stream stream);

/* Memory-bank projection (csrc/project.hip).
 * pio_test_project_pass: ONE bank pass -- k_project2 with `groups` query groups of 16 (1, 2, or 3 at D = 768) on `parts` workgroups, then
 * k_project_combine -- through the function launch_mem_project's loop calls, for the queries q0 .. min(N, q0 + 16 groups) - 1.
 *   split 0: exact fp32 operands (bank_split / bank_scale unread); 1: split fp16 operands, bank_split [M][2][D] fp16 = pio_test_bank_prep's
 *   image of bank * bank_scale (a positive finite power of two that brings max|bank| into [2^14, 2^15))
 *   bank [M][D], inv_norm [M]; q [N][D] UNIT rows (the hook does not normalise); out [N][D]: rows q0 .. of this pass are written
 *   parts 1 .. 1024: the workgroups launched.  Slabs: units of 16 rows (groups 1) or 32 rows (groups 2, 3), ceil(units / parts) units per
 *   workgroup, in order; workgroups past the last unit have an empty slab
 *   part_acc [part_rows][D], part_ml [part_rows][2], part_rows >= parts * 16 groups: workgroup b leaves query n's running maximum m and
 *   sum l = sum_r e^(z_r - m) at part_ml[b * 16 groups + n], Acc = sum_r e^(z_r - m) bank[r] at part_acc[same row]; an empty slab m = -inf
 * Refused with PIO_ERR_INVALID_ARG before any launch: another D, groups 3 at D != 768, split without its image and scale, parts outside
 * 1 .. 1024, part_rows too small, N - q0 < 1, temperature not finite and positive; and split = 1 with one group in a build without the
 * split instance of the 16-query pass (PIO_PROJECT_SPLIT16 = 0): the hook never runs another form than the one asked for. */
int pio_test_project_pass(int32_t groups, int32_t split, const float* bank, const void* bank_split, float bank_scale, const float* inv_norm,
                          int64_t M, int32_t D, const float* q, int32_t N, int32_t q0, float temperature, int32_t parts, float* part_acc,
                          float* part_ml, int32_t part_rows, float* out, pio_stream stream);
/* What loading a bank computes, on caller-owned buffers; a NULL output skips its step.  inv_norm [M] = 1 / |bank[r]|; abs_max [1]: the bit
 * pattern of max |bank| (a non-negative float); bank_split [M][2][D] fp16: hi = fp16(x scale), lo = fp16(x scale - hi). */
int pio_test_bank_prep(const float* bank, int64_t M, int32_t D, float scale, float* inv_norm, uint32_t* abs_max, void* bank_split, pio_stream stream);

/* stop_at_eos bookkeeping (dec_stop.hip) on caller-owned device buffers.  ids [N][steps] int32, N <= 256, steps <= 64, 0 <= s0 < s1 <= steps.
 * scan: first[n] = first column in [s0, s1) of row n that holds stop0 or stop1 (stop1 < 0: none), unless first[n] already names a column
 *   before s0, which is kept (`steps`: no stop; at s0 == 0 the incoming first[] is ignored); *live = rows without a stop.  Columns outside
 *   [s0, s1) are not read.
 * pad: out [N][steps] = ids with every column after first[n] set to ids[n][first[n]] (out != ids). */
int pio_test_dec_stop_scan(const int32_t* ids, int32_t N, int32_t steps, int32_t s0, int32_t s1, int32_t stop0, int32_t stop1, int32_t* first,
                           int32_t* live, pio_stream stream);
int pio_test_dec_stop_pad(const int32_t* ids, const int32_t* first, int32_t N, int32_t steps, int32_t* out, pio_stream stream);

/* The exact-fp32 kernels, one launch per call, all pointers DEVICE fp32 unless said otherwise; no call synchronises.
 * pio_test_sgemm (k_sgemm_tn): C [M][ldc] = alpha * A [M][lda] . W [N][ldw]^T (+ bias [N], may be NULL) (relu) (resid: + the old C).
 *   Columns n >= N of C and rows m >= M are never written.  A and W 16-byte aligned; lda, ldw >= K; ldc >= N.  The launcher refuses K < 32,
 *   K % 32 != 0, lda % 4 != 0, ldw % 4 != 0 and relu with resid: PIO_ERR_INVALID_ARG, nothing launched. */
int pio_test_sgemm(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, float alpha, float* C, int32_t ldc, int32_t M,
                   int32_t N, int32_t K, int32_t relu, int32_t resid, pio_stream stream);
/* qkv [B*Tp][3D] (q | k | v along a row, head h in columns [64 h, 64 h + 64) of each third), D == 64 H -> out [B*Tp][D].
 * kind 0 (k_attention_f32): sequence b attends its first len keys, len = lens[b] (DEVICE [B] int32, the caller keeps 0 <= lens[b] <= Tp;
 *   not read back) or T without lens; rows len <= t < Tp are written as zero.  kind 1 (k_text_attention_f32): causal, query t attends
 *   keys 0 .. t; takes no lens, T ignored. */
int pio_test_attention_f32(int32_t kind, const float* qkv, int32_t B, int32_t H, int32_t T, int32_t Tp, int32_t D, float scale,
                           const int32_t* lens, float* out, pio_stream stream);
/* k_layernorm_f32: y [M][D] = LayerNorm(x [M][D]) * w + b (biased variance, eps under the root); y == x is allowed (the CLIP pre-norm) */
int pio_test_layernorm_f32(const float* x, const float* w, const float* b, float eps, int32_t M, int32_t D, float* y, pio_stream stream);
enum {
  PIO_POINTWISE_GELU_ERF = 0,      /* y = 0.5 y (1 + erf(y / sqrt 2))      k_gelu_f32 act 0 */
  PIO_POINTWISE_QUICKGELU = 1,     /* y = y / (1 + exp(-1.702 y))          k_gelu_f32 act 1 */
  PIO_POINTWISE_TANH = 2,          /* y = tanh(y)                          k_activation_f32 act 2 */
  PIO_POINTWISE_SIGMOID = 3,       /* y = 1 / (1 + exp(-y))                k_activation_f32 act 3 */
  PIO_POINTWISE_RESID_LS = 4       /* y[i] += aux[i] * ls[i % D]           k_resid_ls_f32 (aux [n], ls [D]; ops 0..3 ignore aux, ls, D) */
};
/* in place on y [n], 1 <= n <= 2^31 */
int pio_test_pointwise_f32(int32_t op, float* y, int64_t n, const float* aux, const float* ls, int32_t D, pio_stream stream);
/* k_im2col_f32: imgs [B][3][S][S] -> out [B (S/p)^2][Kpad], column c p^2 + py p + px; the columns >= 3 p^2 are NOT written (the forward
 * zero-fills its buffer once, at creation) */
int pio_test_im2col_f32(const float* imgs, int32_t B, int32_t S, int32_t p, int32_t Kpad, float* out, pio_stream stream);
/* k_embed_scatter_f32: x [B*Tp][D] rows b Tp + G + i = emb [B*n2][D] row b n2 + i + pos [1 + n2][D] row 1 + i; other rows not written */
int pio_test_embed_scatter_f32(const float* emb, const float* pos, int32_t B, int32_t n2, int32_t Tp, int32_t G, int32_t D, float* x,
                               pio_stream stream);
/* k_text_embed: ids [N][L] int32 -> x [N*Tp][W] = tok [V][W] row id + pos [>= L][W] row t; rows t >= L zero.  An id outside [0, V) gives a
 * zero row and ORs 1 into *err (DEVICE int32, zeroed by the caller).  Tp >= L, Tp % 8 == 0. */
int pio_test_text_embed(const int32_t* ids, int32_t N, int32_t L, int32_t Tp, int32_t V, int32_t W, const float* tok, const float* pos, float* x,
                        int32_t* err, pio_stream stream);
/* k_text_pool: out [N][E] = LayerNorm(x [N*Tp][W] row s Tp + (first arg-max of ids [N][L] row s); lw, lb [W], eps) . proj [W][E]; W <= 1024 */
int pio_test_text_pool(const float* x, const int32_t* ids, int32_t N, int32_t L, int32_t Tp, int32_t W, int32_t E, const float* lw,
                       const float* lb, float eps, const float* proj, float* out, pio_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PATCHIONER_HIP_H */
