// C ABI of the CLIP text tower (include/patchioner_hip.h: pio_text_*): a handle of its own, weight packing, the launch plan of
// one encode (text_encoder.hip + the ViT's GEMMs and LayerNorm).
#include "../../include/patchioner_hip.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "host_prep.h"
#include "kernels.h"

using namespace pio;

namespace pio {
int api_fail(int code, const std::string& msg);   // api.cpp: sets pio_last_error's message
}

namespace {

int fail(int code, const std::string& msg) { return api_fail(code, msg); }

#define HIP_OK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess)                                                                         \
      return fail(PIO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                \
  } while (0)

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

}  // namespace

struct pio_text_context {
  pio_text_config cfg;
  int W = 0, H = 0, Tmax = 0, Tk = 0;
  OperandType op = OP_F16;
  bool f32 = false, finalized = false;
  std::unordered_map<std::string, HostTensor> host;
  std::vector<void*> allocs;
  struct Layer {
    float *n1w, *n1b, *qkvb, *projb, *n2w, *n2b, *fc1b, *fc2b;
    void *qkvw, *projw, *fc1w, *fc2w;             // operand type (MFMA path)
    float *qkvw32, *projw32, *fc1w32, *fc2w32;    // fp32 (parity mode)
  };
  std::vector<Layer> layer;
  float *tok = nullptr, *pos = nullptr, *lnf_w = nullptr, *lnf_b = nullptr, *proj = nullptr;
  // workspaces, sized for max_texts captions of Tmax rows
  float* x = nullptr;
  void *xn = nullptr, *ao = nullptr, *hbuf = nullptr, *q = nullptr, *k = nullptr, *vT = nullptr;
  float *f_xn = nullptr, *f_qkv = nullptr, *f_ao = nullptr, *f_h = nullptr;
  int32_t* err_dev = nullptr;
  int32_t* err_host = nullptr;      // pinned

  int dmalloc_bytes(void** p, size_t bytes, bool zero) {
    HIP_OK(hipMalloc(p, bytes > 0 ? bytes : 16));
    allocs.push_back(*p);
    if (zero) HIP_OK(hipMemset(*p, 0, bytes));
    return PIO_OK;
  }
  int upload(const std::vector<float>& v, float** dst) {
    int rc = dmalloc_bytes((void**)dst, v.size() * 4, false);
    if (rc) return rc;
    HIP_OK(hipMemcpy(*dst, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    return PIO_OK;
  }
  int upload_op(const std::vector<float>& v, void** dst) {
    std::vector<uint16_t> tmp(v.size());
    convert_row(op == OP_F16, v.data(), (int64_t)v.size(), tmp.data());
    int rc = dmalloc_bytes(dst, tmp.size() * 2, false);
    if (rc) return rc;
    HIP_OK(hipMemcpy(*dst, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    return PIO_OK;
  }
  int need(const std::string& key, std::vector<int64_t> shape, const HostTensor** out) {
    auto it = host.find(key);
    if (it == host.end()) return fail(PIO_ERR_NOT_READY, "pio_text_finalize: missing weight '" + key + "'");
    if (it->second.shape != shape) {
      std::string want, got;
      for (auto s : shape) want += std::to_string(s) + ",";
      for (auto s : it->second.shape) got += std::to_string(s) + ",";
      return fail(PIO_ERR_SHAPE, "pio_text_finalize: weight '" + key + "' has shape [" + got + "], expected [" + want + "]");
    }
    *out = &it->second;
    return PIO_OK;
  }
};

namespace {

bool text_key_known(const std::string& k, int layers) {
  static const char* top[] = {"token_embedding.weight", "positional_embedding", "ln_final.weight", "ln_final.bias", "text_projection"};
  for (auto t : top)
    if (k == t) return true;
  static const std::string pre = "transformer.resblocks.";
  if (k.rfind(pre, 0) != 0) return false;
  size_t p = pre.size(), e = k.find('.', p);
  if (e == std::string::npos || e == p) return false;
  int l = 0;
  for (size_t i = p; i < e; ++i) {
    if (k[i] < '0' || k[i] > '9') return false;
    l = l * 10 + (k[i] - '0');
  }
  if (l >= layers) return false;
  static const char* sub[] = {"ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias", "attn.in_proj_weight", "attn.in_proj_bias",
                              "attn.out_proj.weight", "attn.out_proj.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
                              "mlp.c_proj.bias"};
  const std::string rest = k.substr(e + 1);
  for (auto s : sub)
    if (rest == s) return true;
  return false;
}

int text_finalize_impl(pio_text_context* c) {
  const int W = c->W, V = c->cfg.vocab_size, C = c->cfg.context_length, E = c->cfg.embed_dim;
  const HostTensor* t;
  int rc;
  if ((rc = c->need("token_embedding.weight", {V, W}, &t)) || (rc = c->upload(t->data, &c->tok))) return rc;
  if ((rc = c->need("positional_embedding", {C, W}, &t)) || (rc = c->upload(t->data, &c->pos))) return rc;
  if ((rc = c->need("ln_final.weight", {W}, &t)) || (rc = c->upload(t->data, &c->lnf_w))) return rc;
  if ((rc = c->need("ln_final.bias", {W}, &t)) || (rc = c->upload(t->data, &c->lnf_b))) return rc;
  if ((rc = c->need("text_projection", {W, E}, &t)) || (rc = c->upload(t->data, &c->proj))) return rc;
  c->layer.assign(c->cfg.layers, pio_text_context::Layer{});
  for (int l = 0; l < c->cfg.layers; ++l) {
    pio_text_context::Layer& L = c->layer[l];
    const std::string pre = "transformer.resblocks." + std::to_string(l) + ".";
    struct F { const char* key; int64_t n; float** dst; };
    F fs[] = {{"ln_1.weight", W, &L.n1w}, {"ln_1.bias", W, &L.n1b}, {"attn.in_proj_bias", 3 * W, &L.qkvb},
              {"attn.out_proj.bias", W, &L.projb}, {"ln_2.weight", W, &L.n2w}, {"ln_2.bias", W, &L.n2b},
              {"mlp.c_fc.bias", 4 * W, &L.fc1b}, {"mlp.c_proj.bias", W, &L.fc2b}};
    for (auto& f : fs)
      if ((rc = c->need(pre + f.key, {f.n}, &t)) || (rc = c->upload(t->data, f.dst))) return rc;
    // the packed nn.MultiheadAttention in_proj [3W][W] (q | k | v rows) is the ViT's qkv Linear; out_proj, c_fc, c_proj are
    // Linear layers in the [out][in] layout the GEMMs take
    struct Wm { const char* key; int64_t rows, cols; void** dst; float** dst32; };
    Wm ws[] = {{"attn.in_proj_weight", 3 * W, W, &L.qkvw, &L.qkvw32}, {"attn.out_proj.weight", W, W, &L.projw, &L.projw32},
               {"mlp.c_fc.weight", 4 * W, W, &L.fc1w, &L.fc1w32}, {"mlp.c_proj.weight", W, 4 * W, &L.fc2w, &L.fc2w32}};
    for (auto& w : ws) {
      if ((rc = c->need(pre + w.key, {w.rows, w.cols}, &t))) return rc;
      if ((rc = c->f32 ? c->upload(t->data, w.dst32) : c->upload_op(t->data, w.dst))) return rc;
    }
  }
  const size_t M = (size_t)c->cfg.max_texts * c->Tmax, BH = (size_t)c->cfg.max_texts * c->H;
  if ((rc = c->dmalloc_bytes((void**)&c->x, M * W * 4, true))) return rc;
  if (c->f32) {
    if ((rc = c->dmalloc_bytes((void**)&c->f_xn, M * W * 4, true))) return rc;
    if ((rc = c->dmalloc_bytes((void**)&c->f_qkv, M * 3 * W * 4, true))) return rc;
    if ((rc = c->dmalloc_bytes((void**)&c->f_ao, M * W * 4, true))) return rc;
    if ((rc = c->dmalloc_bytes((void**)&c->f_h, M * 4 * W * 4, true))) return rc;
  } else {
    if ((rc = c->dmalloc_bytes(&c->xn, M * W * 2, true))) return rc;
    if ((rc = c->dmalloc_bytes(&c->ao, M * W * 2, true))) return rc;
    if ((rc = c->dmalloc_bytes(&c->hbuf, M * 4 * W * 2, true))) return rc;
    if ((rc = c->dmalloc_bytes(&c->q, BH * c->Tk * 64 * 2, true))) return rc;
    if ((rc = c->dmalloc_bytes(&c->k, BH * c->Tk * 64 * 2, true))) return rc;
    if ((rc = c->dmalloc_bytes(&c->vT, BH * c->Tk * 64 * 2, true))) return rc;
  }
  if ((rc = c->dmalloc_bytes((void**)&c->err_dev, 4, true))) return rc;
  HIP_OK(hipHostMalloc((void**)&c->err_host, 4, hipHostMallocDefault));
  HIP_OK(hipDeviceSynchronize());
  c->host.clear();
  return PIO_OK;
}

}  // namespace

extern "C" {

int pio_text_create(const pio_text_config* cfg, pio_text_handle* out) {
  if (!cfg || !out) return fail(PIO_ERR_INVALID_ARG, "pio_text_create: null argument");
  if (cfg->width < 64 || cfg->width % 256 != 0 || cfg->width > 1024 || cfg->heads * 64 != cfg->width)
    return fail(PIO_ERR_INVALID_ARG, "pio_text_create: width must be a multiple of 256 up to 1024 with heads = width / 64");
  if (cfg->layers < 1 || cfg->context_length < 1 || cfg->context_length > 120 || cfg->vocab_size < 1 || cfg->embed_dim < 1 ||
      cfg->max_texts < 1)
    return fail(PIO_ERR_INVALID_ARG, "pio_text_create: layers, vocab_size, embed_dim, max_texts >= 1 and context_length in [1, 120]");
  if (cfg->operand_type != 0 && cfg->operand_type != 2)
    return fail(PIO_ERR_INVALID_ARG, "pio_text_create: operand_type must be 0 (fp16) or 2 (fp32)");
  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail(PIO_ERR_INVALID_ARG, "pio_text_create: no such HIP device");
  pio_text_context* c = new pio_text_context();
  c->cfg = *cfg;
  c->W = cfg->width;
  c->H = cfg->heads;
  c->Tmax = round_up(cfg->context_length, 8);
  c->Tk = round_up(c->Tmax, 64);
  c->f32 = cfg->operand_type == 2;
  c->op = OP_F16;
  *out = c;
  return PIO_OK;
}

int pio_text_destroy(pio_text_handle c) {
  if (!c) return PIO_OK;
  (void)hipSetDevice(c->cfg.device);
  (void)hipDeviceSynchronize();
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->err_host) (void)hipHostFree(c->err_host);
  delete c;
  return PIO_OK;
}

int pio_text_load_weight(pio_text_handle c, const char* key, const float* host_data, const int64_t* shape, int32_t ndim) {
  if (!c || !key || !host_data || ndim < 0 || (ndim > 0 && !shape)) return fail(PIO_ERR_INVALID_ARG, "pio_text_load_weight: null argument");
  if (c->finalized) return fail(PIO_ERR_INVALID_ARG, "pio_text_load_weight: weights already finalized");
  const std::string k(key);
  if (!text_key_known(k, c->cfg.layers)) return fail(PIO_ERR_UNKNOWN_WEIGHT, "pio_text_load_weight: unknown weight key '" + k + "'");
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  if (t.numel() < 0) return fail(PIO_ERR_SHAPE, "pio_text_load_weight: negative extent");
  t.data.assign(host_data, host_data + t.numel());
  c->host[k] = std::move(t);
  return PIO_OK;
}

int pio_text_finalize(pio_text_handle c) {
  if (!c) return fail(PIO_ERR_INVALID_ARG, "pio_text_finalize: null handle");
  if (c->finalized) return fail(PIO_ERR_INVALID_ARG, "pio_text_finalize: called twice");
  HIP_OK(hipSetDevice(c->cfg.device));
  const int rc = text_finalize_impl(c);
  if (rc != PIO_OK) {                         // leave the handle as it was before the call (weights stay loaded)
    (void)hipDeviceSynchronize();
    for (void* p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    if (c->err_host) (void)hipHostFree(c->err_host);
    c->err_host = nullptr;
    return rc;
  }
  c->finalized = true;
  return PIO_OK;
}

int pio_text_encode(pio_text_handle c, const int32_t* ids, int32_t N, int32_t L, float* out, pio_stream stream) {
  if (!c || !ids || !out) return fail(PIO_ERR_INVALID_ARG, "pio_text_encode: null argument");
  if (!c->finalized) return fail(PIO_ERR_NOT_READY, "pio_text_encode: weights not finalized");
  if (N < 1 || N > c->cfg.max_texts)
    return fail(PIO_ERR_CAPACITY, "pio_text_encode: N = " + std::to_string(N) + " outside [1, max_texts = " + std::to_string(c->cfg.max_texts) + "]");
  if (L < 1 || L > c->cfg.context_length)
    return fail(PIO_ERR_SHAPE, "pio_text_encode: L = " + std::to_string(L) + " outside [1, context_length = " + std::to_string(c->cfg.context_length) + "]");
  HIP_OK(hipSetDevice(c->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  const int W = c->W, Tp = round_up(L, 8), M = N * Tp;
  const float eps = 1e-5f, scale = 0.125f;   // head dim 64
  HIP_OK(launch_text_embed(ids, N, L, Tp, c->cfg.vocab_size, W, c->tok, c->pos, c->x, c->err_dev, s));
  if (c->f32) {
    for (const auto& Ly : c->layer) {
      HIP_OK(launch_layernorm_f32(c->x, Ly.n1w, Ly.n1b, eps, M, W, c->f_xn, s));
      HIP_OK(launch_sgemm_tn(c->f_xn, W, Ly.qkvw32, W, Ly.qkvb, 1.f, c->f_qkv, 3 * W, M, 3 * W, W, 0, 0, s));
      HIP_OK(launch_text_attention_f32(c->f_qkv, N, c->H, Tp, W, scale, c->f_ao, s));
      HIP_OK(launch_sgemm_tn(c->f_ao, W, Ly.projw32, W, Ly.projb, 1.f, c->x, W, M, W, W, 0, 1, s));      // x += attn
      HIP_OK(launch_layernorm_f32(c->x, Ly.n2w, Ly.n2b, eps, M, W, c->f_xn, s));
      HIP_OK(launch_sgemm_tn(c->f_xn, W, Ly.fc1w32, W, Ly.fc1b, 1.f, c->f_h, 4 * W, M, 4 * W, W, 0, 0, s));
      HIP_OK(launch_gelu_f32(c->f_h, (size_t)M * 4 * W, 1, s));
      HIP_OK(launch_sgemm_tn(c->f_h, 4 * W, Ly.fc2w32, 4 * W, Ly.fc2b, 1.f, c->x, W, M, W, 4 * W, 0, 1, s));   // x += mlp
    }
  } else {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.T = Tp; g.Tp = Tp; g.Tk = c->Tk; g.G = 0; g.n2 = 0; g.D = W; g.H = c->H;
    g.x = c->x; g.q = c->q; g.k = c->k; g.vT = c->vT;
    VitAttnArgs at;
    at.q = c->q; at.k = c->k; at.vT = c->vT; at.out = c->ao; at.B = N; at.H = c->H; at.T = Tp; at.Tp = Tp; at.Tk = c->Tk; at.D = W;
    at.scale = scale;
    for (size_t l = 0; l < c->layer.size(); ++l) {
      const auto& Ly = c->layer[l];
      HIP_OK(launch_layernorm(c->op, c->x, Ly.n1w, Ly.n1b, eps, M, W, c->xn, nullptr, Tp, Tp, s));
      {
        GemmArgs a = g;
        a.A = c->xn; a.lda = W; a.W = Ly.qkvw; a.bias = Ly.qkvb; a.M = M; a.N = 3 * W; a.K = W;
        HIP_OK(launch_vit_gemm(c->op, EPI_QKV, a, s));
      }
      HIP_OK(launch_text_attention(c->op, at, s));
      {
        GemmArgs a = g;
        a.A = c->ao; a.lda = W; a.W = Ly.projw; a.bias = Ly.projb; a.M = M; a.N = W; a.K = W;
        HIP_OK(launch_vit_gemm(c->op, EPI_RESIDUAL, a, s));
      }
      HIP_OK(launch_layernorm(c->op, c->x, Ly.n2w, Ly.n2b, eps, M, W, c->xn, nullptr, Tp, Tp, s));
      {
        GemmArgs a = g;
        a.A = c->xn; a.lda = W; a.W = Ly.fc1w; a.bias = Ly.fc1b; a.out16 = c->hbuf; a.M = M; a.N = 4 * W; a.K = W; a.act = 1;
        HIP_OK(launch_vit_gemm(c->op, EPI_GELU, a, s));
      }
      {
        GemmArgs a = g;
        a.A = c->hbuf; a.lda = 4 * W; a.W = Ly.fc2w; a.bias = Ly.fc2b; a.M = M; a.N = W; a.K = 4 * W;
        HIP_OK(launch_vit_gemm(c->op, EPI_RESIDUAL, a, s));
      }
    }
  }
  HIP_OK(launch_text_pool(c->x, ids, N, L, Tp, W, c->cfg.embed_dim, c->lnf_w, c->lnf_b, eps, c->proj, out, s));
  // the embedding kernel's verdict on the ids: read back, cleared for the next call
  HIP_OK(hipMemcpyAsync(c->err_host, c->err_dev, 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemsetAsync(c->err_dev, 0, 4, s));
  HIP_OK(hipStreamSynchronize(s));
  if (*c->err_host != 0)
    return fail(PIO_ERR_INVALID_ARG, "pio_text_encode: a token id outside [0, vocab_size = " + std::to_string(c->cfg.vocab_size) +
                                         ") (its row was zeroed; the output is not valid)");
  return PIO_OK;
}

}  // extern "C"
