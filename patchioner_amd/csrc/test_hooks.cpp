// C ABI test hooks (include/patchioner_hip.h, "Test hooks"): one ViT block kernel, one decoder layer GEMM / attention launch, one beam
// selection / bookkeeping step / head pass, one bank pass of the memory projection, or one exact-fp32 kernel (GEMM, attention, LayerNorm,
// pointwise, im2col / scatter, text embed / pool), per call on caller-owned device buffers, for the kernel-by-kernel tests.
// A translation unit of its own: the host-only AddressSanitizer build (tests/test_asan_host.py) is api.cpp alone against a stub of every
// launcher that api.cpp calls (tests/hipstub/hip_stub.cpp), and these hooks call launchers that api.cpp does not.
#include "../../include/patchioner_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "common.h"
#include "kernels.h"

using namespace pio;

namespace pio {
int api_fail(int code, const std::string& msg);   // api.cpp: sets pio_last_error's message
}  // namespace pio

namespace {

int fail(int code, const std::string& msg) { return api_fail(code, msg); }

GemmArgs test_gemm_args(const pio_test_gemm_args& t) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = t.A; g.W = t.W; g.bias = t.bias; g.M = t.M; g.N = t.N; g.K = t.K; g.lda = t.lda;
  g.x = t.x; g.pos = t.pos; g.out16 = t.out16; g.q = t.q; g.k = t.k; g.vT = t.vT; g.qkv_last = t.qkv_last;
  g.T = t.T; g.Tp = t.Tp; g.Tk = t.Tk; g.G = t.G; g.n2 = t.n2; g.D = t.D; g.H = t.H; g.act = t.act;
  g.pf = t.pf; g.pf_bytes = t.pf_bytes;
  return g;
}

// the sizes every kernel of the epilogue relies on (the forward passes hold them by construction); "" when they hold
std::string test_gemm_shape_error(int32_t epi, const pio_test_gemm_args& t, bool route_only) {
  if (t.M < 1 || t.N < 1 || t.K < 1 || t.lda < t.K || t.lda % 8 != 0) return "M, N, K >= 1, lda >= K, lda % 8 == 0";
  if (!route_only && (!t.A || !t.W || !t.bias)) return "null A, W or bias";
  if (!route_only && (t.pf_bytes < 0 || (t.pf_bytes > 0 && !t.pf))) return "pf_bytes > 0 needs pf";
  switch (epi) {
    case PIO_GEMM_EPI_PATCH_EMBED:
      if (t.N != t.D || t.n2 < 1 || t.M % t.n2 != 0 || t.G < 0 || t.Tp < t.G + t.n2) return "patch embed: N == D, M % n2 == 0, Tp >= G + n2";
      if (!route_only && (!t.x || !t.pos)) return "patch embed: null x or pos";
      return "";
    case PIO_GEMM_EPI_QKV:
      if (t.H < 1 || t.D != 64 * t.H || t.D % 128 != 0 || t.N != 3 * t.D) return "qkv: D == 64 H, D % 128 == 0, N == 3 D";
      if (t.Tp < 8 || t.Tp % 8 != 0 || t.M % t.Tp != 0 || t.Tk < t.Tp || t.Tk % 8 != 0) return "qkv: Tp % 8 == 0, M % Tp == 0, Tk >= Tp, Tk % 8 == 0";
      if (t.qkv_last && (t.T < 1 || t.T > t.Tp)) return "qkv: capture needs 1 <= T <= Tp";
      if (!route_only && (!t.q || !t.k || !t.vT)) return "qkv: null q, k or vT";
      return "";
    case PIO_GEMM_EPI_RESIDUAL:
      if (t.N != t.D) return "residual: N == D";
      if (!route_only && !t.x) return "residual: null x";
      return "";
    case PIO_GEMM_EPI_GELU:
      if (t.act != 0 && t.act != 1) return "gelu: act 0 or 1";
      if (!route_only && !t.out16) return "gelu: null out16";
      return "";
  }
  return "epi outside 0..3";
}

}  // namespace

extern "C" {

int pio_test_vit_gemm(int32_t operand, int32_t epi, int32_t path, const pio_test_gemm_args* args, int32_t* path_taken, pio_stream stream) {
  if (path_taken) *path_taken = -1;
  if (!args) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_gemm: null args");
  if (operand != 0 && operand != 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_gemm: operand 0 (fp16) or 1 (bf16)");
  if (path < PIO_GEMM_PATH_AUTO || path > PIO_GEMM_PATH_ROLL) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_gemm: path outside 0..5");
  const std::string err = test_gemm_shape_error(epi, *args, false);
  if (!err.empty()) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_gemm: " + err);
  const GemmArgs g = test_gemm_args(*args);
  const int p = path == PIO_GEMM_PATH_AUTO ? route_vit_gemm((GemmEpilogue)epi, g) : path;
  if (p < 0) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_gemm: no kernel takes these sizes");
  const hipError_t e = launch_vit_gemm_path(operand == 1 ? OP_BF16 : OP_F16, (GemmEpilogue)epi, (GemmPath)p, g, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_gemm: path " + std::to_string(p) + " refuses epilogue " + std::to_string(epi) +
                                         " at M " + std::to_string(g.M) + ", N " + std::to_string(g.N) + ", K " + std::to_string(g.K));
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_vit_gemm: ") + hipGetErrorString(e));
  if (path_taken) *path_taken = p;
  return PIO_OK;
}

int pio_test_gemm_route(int32_t epi, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t D, int32_t Tp, int32_t has_capture) {
  pio_test_gemm_args t;
  memset(&t, 0, sizeof(t));
  t.M = M; t.N = N; t.K = K; t.lda = lda; t.D = D; t.Tp = Tp; t.T = Tp; t.Tk = round_up(Tp, 64); t.H = D / 64; t.act = 0;
  t.n2 = 1; t.G = 0;                                          // the route does not depend on the image layout
  t.qkv_last = has_capture ? (float*)&t : nullptr;        // only its presence is read
  const std::string err = test_gemm_shape_error(epi, t, true);
  if (!err.empty()) return fail(PIO_ERR_INVALID_ARG, "pio_test_gemm_route: " + err);
  const int p = route_vit_gemm((GemmEpilogue)epi, test_gemm_args(t));
  if (p < 0) return fail(PIO_ERR_INVALID_ARG, "pio_test_gemm_route: no kernel takes these sizes");
  return p;
}

int pio_test_vit_vonly(int32_t operand, int32_t path, const void* A, const void* in_proj_w, const float* in_proj_b, void* out16, int32_t M,
                       int32_t D, int32_t* path_taken, pio_stream stream) {
  if (path_taken) *path_taken = -1;
  if (operand != 0 && operand != 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_vonly: operand 0 (fp16) or 1 (bf16)");
  if (!A || !in_proj_w || !in_proj_b || !out16) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_vonly: null buffer");
  if (M < 1 || D < 256 || D % 256 != 0) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_vonly: M >= 1, D a multiple of 256");
  if (path != PIO_GEMM_PATH_AUTO && path != PIO_GEMM_PATH_WIDE128 && path != PIO_GEMM_PATH_K256)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_vonly: the V-only epilogue exists on paths 3 (WIDE128) and 4 (K256) only");
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.lda = D; g.M = M; g.N = D; g.K = D; g.D = D; g.H = D / 64; g.Tp = 8; g.T = 8; g.Tk = 64;
  g.W = (const char*)in_proj_w + (size_t)2 * D * D * 2;       // rows [2D, 3D) of the fused weight (two bytes per element)
  g.bias = in_proj_b + 2 * D;
  g.out16 = out16;
  const int p = path == PIO_GEMM_PATH_AUTO ? route_vit_gemm(EPI_BIAS, g) : path;
  if (p < 0) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_vonly: no kernel takes these sizes");
  const hipError_t e = launch_vit_gemm_path(operand == 1 ? OP_BF16 : OP_F16, EPI_BIAS, (GemmPath)p, g, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_vit_vonly: path " + std::to_string(p) + " refuses M " + std::to_string(M) + ", D " + std::to_string(D));
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_vit_vonly: ") + hipGetErrorString(e));
  if (path_taken) *path_taken = p;
  return PIO_OK;
}

int pio_test_attention(int32_t kind, int32_t operand, const void* q, const void* k, const void* vT, void* out, int32_t B, int32_t H,
                       int32_t T, int32_t Tp, int32_t Tk, int32_t D, float scale, const int32_t* lens, pio_stream stream) {
  if (kind != 0 && kind != 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention: kind 0 (ViT) or 1 (text, causal)");
  if (operand != 0 && operand != 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention: operand 0 (fp16) or 1 (bf16)");
  if (!q || !k || !vT || !out) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention: null buffer");
  if (B < 1 || H < 1 || D != 64 * H || Tp < 1 || Tp % 8 != 0 || Tk < Tp || !(scale > 0.f) || !std::isfinite(scale))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_attention: B, H >= 1, D == 64 H, Tp % 8 == 0, Tk >= Tp, finite scale > 0");
  if (kind == 0 && (T < 1 || T > Tp || Tk % 64 != 0))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_attention: ViT attention needs 1 <= T <= Tp and Tk % 64 == 0");
  if (kind == 1 && (lens || round_up(Tp, 32) > 128 || Tk < round_up(Tp, 32) || Tk % 8 != 0))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_attention: text attention needs no lens, round_up(Tp, 32) <= min(Tk, 128), Tk % 8 == 0");
  VitAttnArgs a;
  a.q = q; a.k = k; a.vT = vT; a.out = out; a.B = B; a.H = H; a.T = kind == 0 ? T : Tp; a.Tp = Tp; a.Tk = Tk; a.D = D; a.scale = scale;
  a.lens = kind == 0 ? lens : nullptr;
  const OperandType t = operand == 1 ? OP_BF16 : OP_F16;
  const hipError_t e = kind == 0 ? launch_vit_attention(t, a, (hipStream_t)stream) : launch_text_attention(t, a, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_attention: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_layernorm(int32_t operand, const float* x, const float* w, const float* b, float eps, int32_t M, int32_t D, void* out16,
                       float* out32, int32_t T, int32_t Tp, pio_stream stream) {
  if (operand != 0 && operand != 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_layernorm: operand 0 (fp16) or 1 (bf16)");
  if (!x || !w || !b || (out16 == nullptr) == (out32 == nullptr))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_layernorm: x, w, b and exactly one of out16 / out32");
  if (M < 1 || D < 4 || D % 4 != 0 || D > 1024 || !(eps > 0.f))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_layernorm: M >= 1, D % 4 == 0, 4 <= D <= 1024, eps > 0");
  if (out32 && (Tp < 1 || T < 1 || T > Tp || M % Tp != 0))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_layernorm: out32 needs 1 <= T <= Tp and M % Tp == 0");
  const hipError_t e = launch_layernorm(operand == 1 ? OP_BF16 : OP_F16, x, w, b, eps, M, D, out16, out32, T, Tp, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_layernorm: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_layernorm: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_im2col_alpha(int32_t operand, const float* imgs, const int32_t* img_of_region, const uint8_t* masks, int32_t R, int32_t S,
                          int32_t p, int32_t Kpad, void* out, pio_stream stream) {
  if (operand < 0 || operand > 2) return fail(PIO_ERR_INVALID_ARG, "pio_test_im2col_alpha: operand 0 (fp16), 1 (bf16) or 2 (fp32)");
  if (!imgs || !out || R < 1 || p < 1 || S < p || S % p != 0 || Kpad < 4 * p * p)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_im2col_alpha: imgs, out, R >= 1, S a multiple of p, Kpad >= 4 p^2");
  const hipError_t e = launch_im2col_alpha(operand, imgs, img_of_region, masks, R, S, p, S / p, Kpad, out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_im2col_alpha: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_im2col_alpha: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_conv(int32_t operand, const void* x, const void* w, const float* scale, const float* shift, const void* res, void* y,
                  float* y32, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ks, int32_t stride, int32_t relu,
                  int32_t tile, pio_stream stream) {
  if (operand < 0 || operand > 2) return fail(PIO_ERR_INVALID_ARG, "pio_test_conv: operand 0 (fp16), 1 (bf16) or 2 (fp32)");
  if (!x || !w || !scale || !shift || (y == nullptr) == (y32 == nullptr) || (y32 && res))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_conv: x, w, scale, shift and exactly one of y / y32 (y32: no residual)");
  if (B < 1 || H < 1 || W < 1 || Cin < 8 || Cin % 8 != 0 || Cout < 1 || (ks != 1 && ks != 3) || stride < 1 || tile < 0 || tile > 2)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_conv: B, H, W >= 1, Cin % 8 == 0, ks 1 or 3, stride >= 1, tile 0..2");
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.res = res; a.y = y; a.y32 = y32;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.ks = ks; a.stride = stride; a.pad = ks / 2;
  a.Ho = (H + 2 * a.pad - ks) / stride + 1; a.Wo = (W + 2 * a.pad - ks) / stride + 1; a.relu = relu;
  if (y32) { a.out_f32 = 1; a.out_rows = a.Ho * a.Wo; a.out_off = 0; a.valid = a.Ho * a.Wo; }
  const hipError_t e = launch_conv(operand, a, tile, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_conv: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_conv: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_avgpool(int32_t operand, const void* x, int32_t B, int32_t H, int32_t W, int32_t C, void* y, pio_stream stream) {
  if (operand < 0 || operand > 2 || !x || !y || B < 1 || H < 2 || W < 2 || C < 1)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_avgpool: operand 0..2, x, y, B >= 1, H, W >= 2, C >= 1");
  const hipError_t e = launch_avgpool2(operand, x, B, H, W, C, y, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_avgpool: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_attnpool_in(int32_t operand, const void* x, const float* pos, int32_t B, int32_t HW, int32_t C, int32_t Tp, void* out,
                         pio_stream stream) {
  if (operand < 0 || operand > 2 || !x || !pos || !out || B < 1 || HW < 1 || C < 1 || Tp < HW + 1)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_attnpool_in: operand 0..2, x, pos, out, B, HW, C >= 1, Tp > HW");
  const hipError_t e = launch_attnpool_in(operand, x, pos, B, HW, C, Tp, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_attnpool_in: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_nucleus_sample(const float* scores, int32_t N, int32_t V, float temperature, float top_p, const float* uniforms, int32_t stop_id,
                            int32_t* active, int32_t* tokens, int32_t* kept, pio_stream stream) {
  if (!scores || !uniforms || !active || !tokens || N < 1 || V < 1)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_nucleus_sample: scores, uniforms, active, tokens, N >= 1, V >= 1");
  SampleArgs a;
  a.scores = scores; a.N = N; a.V = V; a.ld = V; a.temperature = temperature; a.top_p = top_p; a.uniforms = uniforms; a.u_stride = 1;
  a.stop_id = stop_id; a.active = active; a.tokens = tokens; a.tok_stride = 1; a.kept = kept;
  const hipError_t e = launch_nucleus_sample(a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_nucleus_sample: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_dec_workspace(int64_t* ws_floats, int32_t* ticket_words) {
  if (!ws_floats || !ticket_words) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_workspace: null output");
  *ws_floats = (int64_t)dec_splitk_ws_floats();
  *ticket_words = DEC_TICKET_WORDS;
  return PIO_OK;
}

int pio_test_dec_split_weights(const float* W, int64_t n, void* out, float* unscale, pio_stream stream) {
  if (!W || !out || !unscale || n < 8 || n % 8 != 0) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_split_weights: W, out, unscale, n a positive multiple of 8");
  const hipError_t e = dec_split_weights(W, (size_t)n, out, unscale, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_split_weights: weights are not finite");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_dec_split_weights: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_dec_gemm(int32_t selector, int32_t epi, const float* W, const void* Wsplit, float unscale, const float* X, int32_t N, int32_t Nout,
                      int32_t K, const float* bias, const float* cvec, const float* extra, float eps, float* out, float* ws, uint32_t* tickets,
                      pio_stream stream) {
  if (selector < PIO_DEC_GEMMS_FAMILY_A || selector > PIO_DEC_GEMMS_BY_ROWS_SPLIT) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_gemm: selector outside 0..3");
  if (!W || !X || !bias || !out) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_gemm: null W, X, bias or out");
  if (N < 1 || N > DEC_MAX_PREFIXES) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_gemm: 1 <= N <= 256");
  bool ok = false;
  switch (epi) {
    case PIO_DEC_EPI_STORE_LN: ok = Nout == 2304 && K == 768 && cvec && eps > 0.f; break;
    case PIO_DEC_EPI_GELU_LN: ok = Nout == 3072 && K == 768 && cvec && eps > 0.f; break;
    case PIO_DEC_EPI_RESID: ok = Nout == 768 && (K == 768 || (K == 3072 && ws && tickets)); break;
    case PIO_DEC_EPI_EMBED: ok = Nout == 768 && (K == 384 || K == 512 || K == 640 || K == 768 || K == 1024) && extra && !Wsplit; break;
    default: return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_gemm: epi outside 0..3");
  }
  if (!ok)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_gemm: epi " + std::to_string(epi) + " refuses Nout " + std::to_string(Nout) + ", K " + std::to_string(K) +
                                         " (or lacks cvec / eps > 0, extra, or the split-K workspace and tickets)");
  if (Wsplit && !(unscale > 0.f && std::isfinite(unscale))) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_gemm: Wsplit needs a finite unscale > 0");
  const bool splitk = K == 3072;     // as in dec_layers: mlp.c_proj, and no other GEMM, gets the workspace
  const hipError_t e = dec_test_layer_gemm(selector, epi, W, X, N, Nout, K, bias, out, extra, cvec, eps, splitk ? ws : nullptr, splitk ? tickets : nullptr,
                                           Wsplit, unscale, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_gemm: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_dec_gemm: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_dec_attention(int32_t form, const float* qkv, float* kcache, float* vcache, float* att, int32_t N, int32_t heads, int32_t max_steps,
                           int32_t pos, int32_t P, const int32_t* plen, int32_t split, const int32_t* tab, int32_t tstride, pio_stream stream) {
  constexpr int E = 768;
  if (form < PIO_DEC_ATTN_STEP || form > PIO_DEC_ATTN_MASK2) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: form outside 0..5");
  if (!qkv || !kcache || !vcache || !att) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: null buffer");
  if (heads < 1 || E % heads != 0 || (E / heads) % 32 != 0 || E / heads > 256)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: 768 / heads must be a multiple of 32, at most 256");
  if (N < 1 || N > 4096 || max_steps < 1 || max_steps > 256) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: 1 <= N <= 4096, 1 <= max_steps <= 256");
  const bool prefill = form == PIO_DEC_ATTN_PREFILL || form == PIO_DEC_ATTN_MASK1 || form == PIO_DEC_ATTN_MASK2;
  const bool ragged = form == PIO_DEC_ATTN_RAGGED || form == PIO_DEC_ATTN_RAGGED_TAB;
  if (prefill && (P < 1 || P > max_steps)) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: prefill needs 1 <= P <= max_steps");
  if (!prefill && (pos < 0 || pos >= max_steps)) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: 0 <= pos < max_steps");
  if ((ragged || form == PIO_DEC_ATTN_MASK1 || form == PIO_DEC_ATTN_MASK2) && !plen) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: this form needs plen");
  if (ragged) {
    std::string lens(sizeof(int32_t) * (size_t)N, '\0');
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(&lens[0], plen, lens.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_dec_attention: ") + hipGetErrorString(e));
    int top = 0;
    for (int n = 0; n < N; ++n) {
      int32_t v;
      memcpy(&v, &lens[sizeof(int32_t) * (size_t)n], sizeof(v));
      if (v < 0 || v + pos >= max_steps) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: 0 <= plen[n], plen[n] + pos < max_steps");
      top = v + pos > top ? v + pos : top;
    }
    if (form == PIO_DEC_ATTN_RAGGED_TAB && (!tab || tstride < top || tstride < 1))
      return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: the tab form needs tab and tstride >= every row's position");
  }
  const hipError_t e = dec_test_attention(form, qkv, kcache, vcache, att, E, heads, N, max_steps, pos, P, plen, split, tab, tstride, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_attention: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_dec_attention: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_beam_select(const float* lp, const float* scores, const float* lens, const int32_t* stopped, int32_t W, int32_t V, float* out_val,
                         int64_t* out_idx, pio_stream stream) {
  if (!lp || !out_val || !out_idx) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_select: null lp, out_val or out_idx");
  if (scores && (!lens || !stopped)) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_select: scores go with lens and stopped");
  if (W < 1 || W > 8 || V < W) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_select: 1 <= W <= 8, V >= W");
  const hipError_t e = launch_beam_select(lp, scores, lens, stopped, W, V, out_val, out_idx, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_select: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_beam_select: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_beam_step(const float* lp, int32_t N, int32_t W, int32_t V, int32_t step, int32_t eos0, int32_t eos1, const int32_t* prow, float* scores,
                       float* lens, int32_t* stopped, int32_t* tok, int32_t* hist, int32_t steps, int32_t* tab, int32_t tstride, const float* wte,
                       const float* wpe, int32_t npos, int32_t E, float* x, pio_stream stream) {
  if (!lp || !prow || !scores || !lens || !stopped || !tok || !hist || !tab || !wte || !wpe || !x)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_step: null buffer");
  if (N < 1 || N > 128 || W < 1 || W > 8 || V < W) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_step: 1 <= N <= 128, 1 <= W <= 8, V >= W");
  if (steps < 1 || steps > 64 || step < 0 || step >= steps) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_step: 1 <= steps <= 64, 0 <= step < steps");
  if (tstride < 1 || tstride > 256 || npos < 1 || E < 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_step: 1 <= tstride <= 256, npos >= 1, E >= 1");
  {
    std::string rows(sizeof(int32_t) * (size_t)N * W, '\0');
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(&rows[0], prow, rows.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_beam_step: ") + hipGetErrorString(e));
    for (int r = 0; r < N * W; ++r) {
      int32_t P;
      memcpy(&P, &rows[sizeof(int32_t) * (size_t)r], sizeof(P));
      if (P < 1 || P + step - 1 >= tstride) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_step: 1 <= prow[r], prow[r] + step - 1 < tstride");
    }
  }
  const hipError_t e = dec_test_beam_step(lp, N, W, V, step, eos0, eos1, prow, scores, lens, stopped, tok, hist, steps, tab, tstride, wte, wpe, npos,
                                          E, x, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_beam_step: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_beam_step: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_lm_head_rows(int32_t kind, const float* head_w, const float* head_c, const float* head_d, float eps, const float* x, int32_t rows,
                          int32_t V, int32_t log_softmax, float* stats, float* out, pio_stream stream) {
  if (kind != 0 && kind != 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_lm_head_rows: kind 0 (LOGITS_FULL) or 1 (LOGITS_ROWS)");
  if (!head_w || !head_c || !head_d || !x || !stats || !out) return fail(PIO_ERR_INVALID_ARG, "pio_test_lm_head_rows: null buffer");
  if (rows < 1 || rows > DEC_MAX_PREFIXES || V < 1 || !(eps > 0.f)) return fail(PIO_ERR_INVALID_ARG, "pio_test_lm_head_rows: 1 <= rows <= 256, V >= 1, eps > 0");
  const hipError_t e = dec_test_lm_head_rows(kind, head_w, head_c, head_d, eps, x, rows, V, log_softmax != 0, stats, out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_lm_head_rows: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_lm_head_rows: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_project_pass(int32_t groups, int32_t split, const float* bank, const void* bank_split, float bank_scale, const float* inv_norm,
                          int64_t M, int32_t D, const float* q, int32_t N, int32_t q0, float temperature, int32_t parts, float* part_acc,
                          float* part_ml, int32_t part_rows, float* out, pio_stream stream) {
  if (!bank || !inv_norm || !q || !part_acc || !part_ml || !out) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: null buffer");
  if (groups < 1 || groups > 3) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: groups 1, 2 or 3");
  if (D != 384 && D != 512 && D != 640 && D != 768 && D != 1024) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: D must be 384, 512, 640, 768 or 1024");
  if (groups == 3 && D != 768) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: the 48-query pass exists at D = 768 only");
  if (split != 0 && split != 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: split 0 (exact fp32) or 1 (split fp16)");
  if (split) {
    int ex = 0;
    const bool pow2 = std::isfinite(bank_scale) && bank_scale > 0.f && std::frexp(bank_scale, &ex) == 0.5f;
    if (!bank_split || !pow2) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: the split form needs bank_split and a positive finite power-of-two scale");
  }
  if (M < 1 || M > ((int64_t)1 << 40)) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: 1 <= M <= 2^40");
  if (q0 < 0 || N - q0 < 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: q0 >= 0 and N - q0 >= 1");
  if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: finite temperature > 0");
  if (parts < 1 || parts > 1024) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: parts outside 1..1024");
  if ((int64_t)part_rows < (int64_t)parts * 16 * groups) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: part_acc / part_ml hold fewer than parts * 16 groups rows");
  ProjectArgs a;
  memset(&a, 0, sizeof(a));
  a.bank = bank; a.inv_norm = inv_norm; a.M = M; a.D = D; a.q = const_cast<float*>(q); a.N = N; a.temperature = temperature; a.out = out;
  a.part_acc = part_acc; a.part_ml = part_ml; a.parts = parts; a.part_rows = part_rows;
  a.bank_scale = split ? bank_scale : 0.f; a.bank_split = split ? bank_split : nullptr;
  if ((split != 0) != project_pass_is_split(a, groups))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: this build has no split instance of the 16-query pass (PIO_PROJECT_SPLIT16 = 0)");
  const hipError_t e = launch_project_pass(a, groups, q0, parts, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_project_pass: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_project_pass: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_bank_prep(const float* bank, int64_t M, int32_t D, float scale, float* inv_norm, uint32_t* abs_max, void* bank_split, pio_stream stream) {
  if (!bank || M < 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_bank_prep: bank and M >= 1");
  if (D != 384 && D != 512 && D != 640 && D != 768 && D != 1024) return fail(PIO_ERR_INVALID_ARG, "pio_test_bank_prep: D must be 384, 512, 640, 768 or 1024");
  if (bank_split && !(scale > 0.f && std::isfinite(scale))) return fail(PIO_ERR_INVALID_ARG, "pio_test_bank_prep: the split image needs a finite scale > 0");
  hipError_t e = hipSuccess;
  if (inv_norm) e = launch_row_inv_norm(bank, M, D, inv_norm, (hipStream_t)stream);
  if (e == hipSuccess && abs_max) e = launch_abs_max(bank, M * D, abs_max, (hipStream_t)stream);
  if (e == hipSuccess && bank_split) e = launch_split_bank(bank, M, D, scale, bank_split, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_bank_prep: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_dec_stop_scan(const int32_t* ids, int32_t N, int32_t steps, int32_t s0, int32_t s1, int32_t stop0, int32_t stop1, int32_t* first,
                           int32_t* live, pio_stream stream) {
  if (!ids || !first || !live) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_stop_scan: null argument");
  if (N < 1 || N > DEC_MAX_PREFIXES || steps < 1 || steps > 64 || s0 < 0 || s1 <= s0 || s1 > steps)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_stop_scan: 1 <= N <= 256, 1 <= steps <= 64, 0 <= s0 < s1 <= steps");
  const hipError_t e = launch_dec_stop_scan(ids, N, steps, s0, s1, stop0, stop1, first, live, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_dec_stop_scan: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_dec_stop_pad(const int32_t* ids, const int32_t* first, int32_t N, int32_t steps, int32_t* out, pio_stream stream) {
  if (!ids || !first || !out || ids == out) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_stop_pad: null argument, or out == ids");
  if (N < 1 || N > DEC_MAX_PREFIXES || steps < 1 || steps > 64) return fail(PIO_ERR_INVALID_ARG, "pio_test_dec_stop_pad: 1 <= N <= 256, 1 <= steps <= 64");
  const hipError_t e = launch_dec_stop_pad(ids, first, N, steps, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_dec_stop_pad: ") + hipGetErrorString(e));
  return PIO_OK;
}

// ---- the exact-fp32 kernels (viecap.hip k_sgemm_tn / k_layernorm_f32 / k_activation_f32, vit_fp32.hip, text_encoder.hip's fp32 side)
int pio_test_sgemm(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, float alpha, float* C, int32_t ldc, int32_t M,
                   int32_t N, int32_t K, int32_t relu, int32_t resid, pio_stream stream) {
  if (!A || !W || !C) return fail(PIO_ERR_INVALID_ARG, "pio_test_sgemm: null A, W or C");
  if (((uintptr_t)A | (uintptr_t)W) % 16 != 0) return fail(PIO_ERR_INVALID_ARG, "pio_test_sgemm: A and W must be 16-byte aligned");
  if (M < 1 || N < 1 || K < 1 || lda < K || ldw < K || ldc < N) return fail(PIO_ERR_INVALID_ARG, "pio_test_sgemm: M, N, K >= 1, lda >= K, ldw >= K, ldc >= N");
  if (!std::isfinite(alpha)) return fail(PIO_ERR_INVALID_ARG, "pio_test_sgemm: finite alpha");
  const hipError_t e = launch_sgemm_tn(A, lda, W, ldw, bias, alpha, C, ldc, M, N, K, relu, resid, (hipStream_t)stream);
  if (e == hipErrorInvalidValue)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_sgemm: refused by the launcher (K >= 32, K % 32 == 0, lda % 4 == 0, ldw % 4 == 0, not relu with resid): K " +
                                         std::to_string(K) + ", lda " + std::to_string(lda) + ", ldw " + std::to_string(ldw) + ", relu " +
                                         std::to_string(relu) + ", resid " + std::to_string(resid));
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_sgemm: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_attention_f32(int32_t kind, const float* qkv, int32_t B, int32_t H, int32_t T, int32_t Tp, int32_t D, float scale,
                           const int32_t* lens, float* out, pio_stream stream) {
  if (kind != 0 && kind != 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention_f32: kind 0 (ViT) or 1 (text, causal)");
  if (!qkv || !out || qkv == out) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention_f32: null buffer, or out == qkv");
  if (B < 1 || H < 1 || D != 64 * H || Tp < 1 || Tp > 4096 || (int64_t)B * H > 65535 || !(scale > 0.f) || !std::isfinite(scale))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_attention_f32: B, H >= 1, B H <= 65535, D == 64 H, 1 <= Tp <= 4096, finite scale > 0");
  if (kind == 0 && (T < 1 || T > Tp)) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention_f32: ViT attention needs 1 <= T <= Tp");
  if (kind == 1 && lens) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention_f32: text attention takes no lens");
  const hipError_t e = kind == 0 ? launch_attention_f32(qkv, B, H, T, Tp, D, scale, lens, out, (hipStream_t)stream)
                                 : launch_text_attention_f32(qkv, B, H, Tp, D, scale, out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_attention_f32: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_attention_f32: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_layernorm_f32(const float* x, const float* w, const float* b, float eps, int32_t M, int32_t D, float* y, pio_stream stream) {
  if (!x || !w || !b || !y) return fail(PIO_ERR_INVALID_ARG, "pio_test_layernorm_f32: null x, w, b or y");
  if (M < 1 || D < 1 || !(eps > 0.f)) return fail(PIO_ERR_INVALID_ARG, "pio_test_layernorm_f32: M >= 1, D >= 1, eps > 0");
  const hipError_t e = launch_layernorm_f32(x, w, b, eps, M, D, y, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_layernorm_f32: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_pointwise_f32(int32_t op, float* y, int64_t n, const float* aux, const float* ls, int32_t D, pio_stream stream) {
  if (op < PIO_POINTWISE_GELU_ERF || op > PIO_POINTWISE_RESID_LS) return fail(PIO_ERR_INVALID_ARG, "pio_test_pointwise_f32: op outside 0..4");
  if (!y || n < 1 || n > ((int64_t)1 << 31)) return fail(PIO_ERR_INVALID_ARG, "pio_test_pointwise_f32: y and 1 <= n <= 2^31");
  hipError_t e;
  if (op == PIO_POINTWISE_RESID_LS) {
    if (!aux || !ls || aux == y || D < 1) return fail(PIO_ERR_INVALID_ARG, "pio_test_pointwise_f32: resid_ls needs aux != y, ls and D >= 1");
    e = launch_resid_ls_f32(y, aux, ls, (size_t)n, D, (hipStream_t)stream);
  } else if (op == PIO_POINTWISE_TANH || op == PIO_POINTWISE_SIGMOID) {
    e = launch_activation_f32(y, (size_t)n, op, (hipStream_t)stream);
  } else {
    e = launch_gelu_f32(y, (size_t)n, op, (hipStream_t)stream);
  }
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_pointwise_f32: refused by the launcher");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_pointwise_f32: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_im2col_f32(const float* imgs, int32_t B, int32_t S, int32_t p, int32_t Kpad, float* out, pio_stream stream) {
  if (!imgs || !out || B < 1 || p < 1 || S < p || S % p != 0 || Kpad < 3 * p * p)
    return fail(PIO_ERR_INVALID_ARG, "pio_test_im2col_f32: imgs, out, B >= 1, S a multiple of p, Kpad >= 3 p^2");
  if ((int64_t)B * 3 * S * S > ((int64_t)1 << 30) || (int64_t)B * (S / p) * (S / p) * Kpad > ((int64_t)1 << 30))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_im2col_f32: at most 2^30 input and 2^30 output elements");
  const hipError_t e = launch_im2col_f32(imgs, B, S, p, S / p, Kpad, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_im2col_f32: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_embed_scatter_f32(const float* emb, const float* pos, int32_t B, int32_t n2, int32_t Tp, int32_t G, int32_t D, float* x,
                               pio_stream stream) {
  if (!emb || !pos || !x) return fail(PIO_ERR_INVALID_ARG, "pio_test_embed_scatter_f32: null emb, pos or x");
  if (B < 1 || n2 < 1 || G < 0 || Tp < G + n2 || D < 1 || (int64_t)B * Tp * D > ((int64_t)1 << 30))
    return fail(PIO_ERR_INVALID_ARG, "pio_test_embed_scatter_f32: B, n2, D >= 1, G >= 0, Tp >= G + n2, B Tp D <= 2^30");
  const hipError_t e = launch_embed_scatter_f32(emb, pos, B, n2, Tp, G, D, x, (hipStream_t)stream);
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_embed_scatter_f32: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_text_embed(const int32_t* ids, int32_t N, int32_t L, int32_t Tp, int32_t V, int32_t W, const float* tok, const float* pos, float* x,
                        int32_t* err, pio_stream stream) {
  if (!ids || !tok || !pos || !x || !err) return fail(PIO_ERR_INVALID_ARG, "pio_test_text_embed: null ids, tok, pos, x or err");
  if (V < 1 || W < 1 || N < 1 || (int64_t)N * Tp > ((int64_t)1 << 24)) return fail(PIO_ERR_INVALID_ARG, "pio_test_text_embed: N, V, W >= 1, N Tp <= 2^24");
  const hipError_t e = launch_text_embed(ids, N, L, Tp, V, W, tok, pos, x, err, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_text_embed: refused by the launcher (N, L >= 1, Tp >= L, Tp % 8 == 0)");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_text_embed: ") + hipGetErrorString(e));
  return PIO_OK;
}

int pio_test_text_pool(const float* x, const int32_t* ids, int32_t N, int32_t L, int32_t Tp, int32_t W, int32_t E, const float* lw,
                       const float* lb, float eps, const float* proj, float* out, pio_stream stream) {
  if (!x || !ids || !lw || !lb || !proj || !out) return fail(PIO_ERR_INVALID_ARG, "pio_test_text_pool: null buffer");
  if (W < 1 || E < 1 || !(eps > 0.f)) return fail(PIO_ERR_INVALID_ARG, "pio_test_text_pool: W >= 1, E >= 1, eps > 0");
  const hipError_t e = launch_text_pool(x, ids, N, L, Tp, W, E, lw, lb, eps, proj, out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(PIO_ERR_INVALID_ARG, "pio_test_text_pool: refused by the launcher (N, L >= 1, W <= 1024, Tp >= L)");
  if (e != hipSuccess) return fail(PIO_ERR_HIP, std::string("pio_test_text_pool: ") + hipGetErrorString(e));
  return PIO_OK;
}

}  // extern "C"
