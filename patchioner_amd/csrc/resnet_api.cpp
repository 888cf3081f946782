// RegionCLIP's ModifiedResNet tower (vit_arch 3): weight packing, NHWC workspaces and the launch plan of one forward
// (resnet.hip's convolutions and pools, the ViT's QKV GEMM and attention kernels for the attnpool).  api.cpp owns the handle; this file
// owns the tower's device memory.
//
// The forward of B images, P/src/regionclip/clip_backbone.py:267-300 (forward_return_spatial_feats with 'res5' in OUT_FEATURES):
//   stem      3 x (3x3 conv + BN + ReLU), the first with stride 2; 2x2 avgpool                      (:237-245)
//   layer1-4  Bottleneck blocks: 1x1 -> 3x3 -> [2x2 avgpool] -> 1x1 + BN3 + identity, ReLU; the identity of a block's first
//             unit is [avgpool] -> 1x1 conv -> BN                                                        (:14-70)
//   attnpool  rows [mean | HW pixels] + position table, q|k|v GEMM, multi-head attention, c_proj on every row (:73-109)
//   tokens    [B][1 + HW][Dout] fp32, each row L2-normalised (F.normalize).  Without attnpool for the spatial features the patch
//             rows are c_proj(x5) (no attention) and row 0 stays the attnpool's.
#include "resnet.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "host_prep.h"
#include "kernels.h"

namespace pio {

int api_fail(int code, const std::string& msg);   // api.cpp: sets pio_last_error's message

namespace {

int fail(int code, const std::string& msg) { return api_fail(code, msg); }

#define HIP_OK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess)                                                                         \
      return fail(PIO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                \
  } while (0)

}  // namespace

struct RnConv {
  void* w = nullptr;             // [Cout][ks][ks][Cin_pad] operand type, or fp32 in the parity mode
  float *scale = nullptr, *shift = nullptr;
  int cin = 0, cin_pad = 0, cout = 0, ks = 1, stride = 1;
};
struct RnBlock {
  RnConv c1, c2, c3, ds;
  bool has_ds = false;
  int stride = 1;
};

struct RnNet {
  int type = 0;                  // 0 fp16, 1 bf16, 2 exact fp32
  int S = 0, width = 0, C = 0, H = 0, Dout = 0, n = 0, T = 0, Tp = 0, Tk = 0, maxB = 0, spatial_attn = 1;
  RnConv stem[3];
  std::vector<RnBlock> blocks;
  float* pos = nullptr;          // [T][C] fp32
  void* qkv_w = nullptr;         // [3C][C] operand type (fp32 in the parity mode)
  float* qkv_b = nullptr;
  RnConv cproj;                  // c_proj as a 1x1 convolution: scale = 1, shift = bias
  void* buf[5] = {};             // NHWC activations, buf_elems elements each
  size_t buf_elems = 0;
  void* apin = nullptr;          // attnpool input [B][Tp][C]
  void *q = nullptr, *k = nullptr, *vT = nullptr, *ao = nullptr;   // MFMA attnpool
  float* f_qkv = nullptr;        // parity mode: [B Tp][3C]
  std::vector<void*> allocs;

  size_t esz() const { return type == 2 ? 4 : 2; }
  int alloc(void** p, size_t bytes) {
    HIP_OK(hipMalloc(p, bytes > 0 ? bytes : 16));
    allocs.push_back(*p);
    HIP_OK(hipMemset(*p, 0, bytes > 0 ? bytes : 16));
    return PIO_OK;
  }
  int upload(const void* src, size_t bytes, void** dst) {
    int rc = alloc(dst, bytes);
    if (rc) return rc;
    HIP_OK(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return PIO_OK;
  }
  // fp32 values -> the operand type's bytes
  int upload_typed(const std::vector<float>& v, void** dst) {
    if (type == 2) return upload(v.data(), v.size() * 4, dst);
    std::vector<uint16_t> t(v.size());
    convert_row(type == 0, v.data(), (int64_t)v.size(), t.data());
    return upload(t.data(), t.size() * 2, dst);
  }
};

namespace {

// torch Conv2d weight [Cout][Cin][ks][ks] -> [Cout][ky][kx][Cin_pad] (zero channels past Cin), plus the BN pair
int load_conv(RnNet* r, const RnGet& get, const std::string& wkey, const std::string& bn, int cin, int cout, int ks, int stride,
              RnConv& cv) {
  cv.cin = cin; cv.cin_pad = round_up(cin, 8); cv.cout = cout; cv.ks = ks; cv.stride = stride;
  const float *w, *sc, *sh;
  int rc;
  if ((rc = get(wkey, (int64_t)cout * cin * ks * ks, &w))) return rc;
  if ((rc = get(bn + ".scale", cout, &sc))) return rc;
  if ((rc = get(bn + ".shift", cout, &sh))) return rc;
  std::vector<float> p((size_t)cout * ks * ks * cv.cin_pad, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < ks * ks; ++t) p[((size_t)o * ks * ks + t) * cv.cin_pad + c] = w[((size_t)o * cin + c) * ks * ks + t];
  if ((rc = r->upload_typed(p, &cv.w))) return rc;
  if ((rc = r->upload(sc, (size_t)cout * 4, (void**)&cv.scale))) return rc;
  return r->upload(sh, (size_t)cout * 4, (void**)&cv.shift);
}

int conv(RnNet* r, const RnConv& cv, const void* x, int B, int H, int W, const void* res, int relu, void* y, hipStream_t s) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = cv.w; a.scale = cv.scale; a.shift = cv.shift; a.res = res; a.y = y;
  a.B = B; a.H = H; a.W = W; a.Cin = cv.cin_pad; a.Cout = cv.cout; a.ks = cv.ks; a.stride = cv.stride; a.pad = cv.ks / 2;
  a.Ho = (H + 2 * a.pad - a.ks) / a.stride + 1; a.Wo = (W + 2 * a.pad - a.ks) / a.stride + 1;
  a.relu = relu;
  HIP_OK(launch_conv(r->type, a, 0, s));
  return PIO_OK;
}

// c_proj on the rows of `x` ([B][rows][C]) into tokens [B][T][Dout] at row out_off + p for p < valid
int cproj(RnNet* r, const void* x, int B, int rows, int out_off, int valid, float* tokens, hipStream_t s) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = r->cproj.w; a.scale = r->cproj.scale; a.shift = r->cproj.shift; a.y32 = tokens;
  a.B = B; a.H = rows; a.W = 1; a.Cin = r->C; a.Cout = r->Dout; a.ks = 1; a.stride = 1; a.Ho = rows; a.Wo = 1;
  a.out_f32 = 1; a.out_rows = r->T; a.out_off = out_off; a.valid = valid;
  HIP_OK(launch_conv(r->type, a, 0, s));
  return PIO_OK;
}

}  // namespace

int rn_build(const pio_config& cfg, const RnGet& get, RnNet** out) {
  *out = nullptr;
  RnNet* r = new RnNet();
  auto done = [&](int rc) -> int {
    if (rc != PIO_OK) { rn_destroy(r); return rc; }
    *out = r;
    return PIO_OK;
  };
  r->type = cfg.vit_operand_type;
  r->S = cfg.crop_dim; r->width = cfg.rn_width; r->C = cfg.embed_dim; r->H = cfg.num_heads;
  r->Dout = cfg.vit_out_dim > 0 ? cfg.vit_out_dim : cfg.embed_dim;
  r->n = cfg.crop_dim / 32; r->T = 1 + r->n * r->n; r->Tp = round_up(r->T, 8); r->Tk = round_up(r->T, 64);
  r->maxB = cfg.max_batch; r->spatial_attn = cfg.rn_attnpool_spatial;
  const int w = r->width, S = r->S, Bm = r->maxB;
  int rc;
  // stem (clip_backbone.py:147-158, 237-245)
  if ((rc = load_conv(r, get, "rn.conv1.weight", "rn.bn1", 3, w / 2, 3, 2, r->stem[0]))) return done(rc);
  if ((rc = load_conv(r, get, "rn.conv2.weight", "rn.bn2", w / 2, w / 2, 3, 1, r->stem[1]))) return done(rc);
  if ((rc = load_conv(r, get, "rn.conv3.weight", "rn.bn3", w / 2, w, 3, 1, r->stem[2]))) return done(rc);
  // the largest activation: the stem's input and outputs, then every block's tensors (the pooled ones are smaller)
  size_t mx = (size_t)S * S * 8;
  mx = std::max(mx, (size_t)(S / 2) * (S / 2) * w);
  int hw = S / 4, inplanes = w;
  for (int L = 0; L < 4; ++L) {
    const int planes = w << L, stride = L == 0 ? 1 : 2;
    for (int i = 0; i < cfg.rn_layers[L]; ++i) {
      RnBlock b;
      b.stride = i == 0 ? stride : 1;
      const std::string pre = "rn.layer" + std::to_string(L + 1) + "." + std::to_string(i) + ".";
      if ((rc = load_conv(r, get, pre + "conv1.weight", pre + "bn1", inplanes, planes, 1, 1, b.c1))) return done(rc);
      if ((rc = load_conv(r, get, pre + "conv2.weight", pre + "bn2", planes, planes, 3, 1, b.c2))) return done(rc);
      if ((rc = load_conv(r, get, pre + "conv3.weight", pre + "bn3", planes, 4 * planes, 1, 1, b.c3))) return done(rc);
      b.has_ds = b.stride > 1 || inplanes != 4 * planes;
      if (b.has_ds &&
          (rc = load_conv(r, get, pre + "downsample.0.weight", pre + "downsample.1", inplanes, 4 * planes, 1, 1, b.ds))) return done(rc);
      mx = std::max(mx, (size_t)hw * hw * std::max(inplanes, 4 * planes));
      hw /= b.stride;
      inplanes = 4 * planes;
      r->blocks.push_back(b);
    }
  }
  if (inplanes != r->C || hw != r->n) { rn_destroy(r); return fail(PIO_ERR_SHAPE, "RegionCLIP tower: layer4 gives " + std::to_string(inplanes) + " channels at " + std::to_string(hw) + "^2, the attnpool takes embed_dim at (crop/32)^2"); }
  // attnpool: q|k|v concatenated at load (weights.regionclip_to_engine), c_proj as a 1x1 conv with unit scale
  const float *pw, *qw, *qb, *cw, *cb;
  const int C = r->C, D = r->Dout;
  if ((rc = get("rn.attnpool.positional_embedding", (int64_t)r->T * C, &pw))) return done(rc);
  if ((rc = get("rn.attnpool.qkv.weight", (int64_t)3 * C * C, &qw))) return done(rc);
  if ((rc = get("rn.attnpool.qkv.bias", (int64_t)3 * C, &qb))) return done(rc);
  if ((rc = get("rn.attnpool.c_proj.weight", (int64_t)D * C, &cw))) return done(rc);
  if ((rc = get("rn.attnpool.c_proj.bias", D, &cb))) return done(rc);
  if ((rc = r->upload(pw, (size_t)r->T * C * 4, (void**)&r->pos))) return done(rc);
  if ((rc = r->upload_typed(std::vector<float>(qw, qw + (size_t)3 * C * C), &r->qkv_w))) return done(rc);
  if ((rc = r->upload(qb, (size_t)3 * C * 4, (void**)&r->qkv_b))) return done(rc);
  r->cproj.cin = r->cproj.cin_pad = C; r->cproj.cout = D;
  if ((rc = r->upload_typed(std::vector<float>(cw, cw + (size_t)D * C), &r->cproj.w))) return done(rc);
  const std::vector<float> ones(D, 1.f);
  if ((rc = r->upload(ones.data(), (size_t)D * 4, (void**)&r->cproj.scale))) return done(rc);
  if ((rc = r->upload(cb, (size_t)D * 4, (void**)&r->cproj.shift))) return done(rc);
  // workspaces for max_batch images
  r->buf_elems = (size_t)Bm * mx;
  for (auto& b : r->buf)
    if ((rc = r->alloc(&b, r->buf_elems * r->esz()))) return done(rc);
  if ((rc = r->alloc(&r->apin, (size_t)Bm * r->Tp * C * r->esz()))) return done(rc);
  if (r->type == 2) {
    if ((rc = r->alloc((void**)&r->f_qkv, (size_t)Bm * r->Tp * 3 * C * 4))) return done(rc);
    if ((rc = r->alloc(&r->ao, (size_t)Bm * r->Tp * C * 4))) return done(rc);
  } else {
    const size_t qk = (size_t)Bm * r->H * r->Tk * 64 * 2;
    if ((rc = r->alloc(&r->q, qk))) return done(rc);
    if ((rc = r->alloc(&r->k, qk))) return done(rc);
    if ((rc = r->alloc(&r->vT, qk))) return done(rc);
    if ((rc = r->alloc(&r->ao, (size_t)Bm * r->Tp * C * 2))) return done(rc);
  }
  HIP_OK(hipDeviceSynchronize());
  return done(PIO_OK);
}

void rn_destroy(RnNet* r) {
  if (!r) return;
  for (void* p : r->allocs) (void)hipFree(p);
  delete r;
}

size_t rn_workspace_bytes(const RnNet* r) { return r ? r->buf_elems * r->esz() * 5 : 0; }

int rn_forward(RnNet* r, const float* imgs, int B, float* tokens, hipStream_t s) {
  const int t = r->type, S = r->S;
  void** bf = r->buf;
  int rc;
  HIP_OK(launch_rn_input(t, imgs, B, S, bf[0], s));
  // stem: buf0 -> buf1 -> buf2 -> buf1 -> avgpool -> buf0
  if ((rc = conv(r, r->stem[0], bf[0], B, S, S, nullptr, 1, bf[1], s))) return rc;
  int hw = S / 2;
  if ((rc = conv(r, r->stem[1], bf[1], B, hw, hw, nullptr, 1, bf[2], s))) return rc;
  if ((rc = conv(r, r->stem[2], bf[2], B, hw, hw, nullptr, 1, bf[1], s))) return rc;
  HIP_OK(launch_avgpool2(t, bf[1], B, hw, hw, r->width, bf[0], s));
  hw /= 2;
  // blocks: x in buf0; conv1 -> buf1, conv2 -> buf2, [avgpool -> buf1]; identity: [avgpool x -> buf3] -> downsample -> buf4; conv3 +
  // identity -> buf0 (with no downsample the identity IS buf0: each element is read by the thread that then writes it)
  for (const RnBlock& b : r->blocks) {
    if ((rc = conv(r, b.c1, bf[0], B, hw, hw, nullptr, 1, bf[1], s))) return rc;
    if ((rc = conv(r, b.c2, bf[1], B, hw, hw, nullptr, 1, bf[2], s))) return rc;
    const void* a = bf[2];
    const int ho = hw / b.stride;
    if (b.stride > 1) {
      HIP_OK(launch_avgpool2(t, bf[2], B, hw, hw, b.c2.cout, bf[1], s));
      a = bf[1];
    }
    const void* idn = bf[0];
    if (b.has_ds) {
      const void* src = bf[0];
      if (b.stride > 1) {
        HIP_OK(launch_avgpool2(t, bf[0], B, hw, hw, b.c1.cin, bf[3], s));
        src = bf[3];
      }
      if ((rc = conv(r, b.ds, src, B, ho, ho, nullptr, 0, bf[4], s))) return rc;
      idn = bf[4];
    }
    if ((rc = conv(r, b.c3, a, B, ho, ho, idn, 1, bf[0], s))) return rc;
    hw = ho;
  }
  // attnpool on x5 = buf0 [B][n^2][C]
  const int C = r->C, HW = r->n * r->n, M = B * r->Tp;
  HIP_OK(launch_attnpool_in(t, bf[0], r->pos, B, HW, C, r->Tp, r->apin, s));
  if (t == 2) {
    HIP_OK(launch_sgemm_tn((const float*)r->apin, C, (const float*)r->qkv_w, C, r->qkv_b, 1.f, r->f_qkv, 3 * C, M, 3 * C, C, 0, 0, s));
    HIP_OK(launch_attention_f32(r->f_qkv, B, r->H, r->T, r->Tp, C, 0.125f, nullptr, (float*)r->ao, s));
  } else {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = r->apin; g.lda = C; g.W = r->qkv_w; g.bias = r->qkv_b; g.M = M; g.N = 3 * C; g.K = C;
    g.q = r->q; g.k = r->k; g.vT = r->vT; g.T = r->T; g.Tp = r->Tp; g.Tk = r->Tk; g.G = 1; g.n2 = HW; g.D = C; g.H = r->H;
    HIP_OK(launch_vit_gemm(t == 0 ? OP_F16 : OP_BF16, EPI_QKV, g, s));
    VitAttnArgs at;
    at.q = r->q; at.k = r->k; at.vT = r->vT; at.out = r->ao; at.B = B; at.H = r->H; at.T = r->T; at.Tp = r->Tp; at.Tk = r->Tk;
    at.D = C; at.scale = 0.125f;
    HIP_OK(launch_vit_attention(t == 0 ? OP_F16 : OP_BF16, at, s));
  }
  if (r->spatial_attn) {
    if ((rc = cproj(r, r->ao, B, r->Tp, 0, r->T, tokens, s))) return rc;
  } else {
    if ((rc = cproj(r, r->ao, B, r->Tp, 0, 1, tokens, s))) return rc;
    if ((rc = cproj(r, bf[0], B, HW, 1, HW, tokens, s))) return rc;
  }
  HIP_OK(launch_l2norm_rows(tokens, B * r->T, r->Dout, s));
  return PIO_OK;
}

}  // namespace pio
