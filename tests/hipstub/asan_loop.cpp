// Drives the C ABI's host side through the create / load / finalize / bank / clone / decode / preprocess / destroy orders
// that crashed an in-process loop on the GPU in round 1 ("Open observations"), on the HIP stub, under
// AddressSanitizer + LeakSanitizer.  Exit code 0 = no finding (ASan aborts otherwise).
// Every entry point of the decodes runs here (hip_stub.cpp stubs every launcher api.cpp calls), and both bounded graph caches are driven past
// their capacity: eviction, eviction after the stream of the last launch has been destroyed, recapture, teardown of populated caches, and one
// injected failure each of hipGraphInstantiate and hipEventCreateWithFlags.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/patchioner_hip.h"

#define CK(x) do { int _rc = (x); if (_rc != PIO_OK) { printf("%s -> %d: %s\n", #x, _rc, pio_last_error()); exit(2); } } while (0)
#define EXPECT_FAIL(x) do { int _rc = (x); if (_rc == PIO_OK) { printf("%s unexpectedly succeeded\n", #x); exit(3); } } while (0)
#define EXPECT_HIP(x) do { int _rc = (x); if (_rc != PIO_ERR_HIP) { printf("%s -> %d, expected PIO_ERR_HIP\n", #x, _rc); exit(5); } } while (0)

// hip_stub.cpp: the next hipGraphInstantiate / hipEventCreateWithFlags fails once
extern "C" void hip_stub_fail_next_graph_instantiate();
extern "C" void hip_stub_fail_next_event_create();

static void load(pio_handle h, const std::string& key, std::vector<int64_t> shape) {
  int64_t n = 1;
  for (auto s : shape) n *= s;
  std::vector<float> v((size_t)n, 0.01f);
  CK(pio_load_weight(h, key.c_str(), v.data(), shape.data(), (int32_t)shape.size()));
}

// kind 0: DeCap (clip_project + GPT-2), 1: ViECap (mapping network + GPT-2), 2: ClipCap (MLP mapper + GPT-2)
static pio_handle make(int kind) {
  const bool viecap = kind == 1;
  pio_config c;
  memset(&c, 0, sizeof(c));
  c.embed_dim = 64; c.depth = 1; c.num_heads = 1; c.patch_size = 14; c.num_registers = 4; c.pretrain_grid = 3; c.crop_dim = 28;
  c.vit_ln_eps = 1e-6f; c.readout_heads = 1; c.readout_scale = 0.125f; c.dec_layers = 1; c.dec_heads = viecap ? 12 : 4; c.dec_embd = 768;
  c.dec_vocab = 64; c.dec_positions = 160; c.prefix_size = 64; c.dec_ln_eps = 1e-5f; c.max_batch = 2; c.max_prefixes = 4;
  c.max_steps = viecap ? 128 : 30; c.vit_operand_type = 0; c.device = 0;
  pio_handle h = nullptr;
  CK(pio_create(&c, &h));
  const int64_t D = 64, E = 768;
  load(h, "cls_token", {1, 1, D}); load(h, "pos_embed", {1, 10, D}); load(h, "register_tokens", {1, 4, D});
  load(h, "patch_embed.proj.weight", {D, 3, 14, 14}); load(h, "patch_embed.proj.bias", {D}); load(h, "norm.weight", {D}); load(h, "norm.bias", {D});
  const char* b = "blocks.0.";
  for (const char* k : {"norm1.weight", "norm1.bias", "attn.proj.bias", "ls1.gamma", "norm2.weight", "norm2.bias", "mlp.fc2.bias", "ls2.gamma"})
    load(h, std::string(b) + k, {D});
  load(h, std::string(b) + "attn.qkv.bias", {3 * D}); load(h, std::string(b) + "mlp.fc1.bias", {4 * D});
  load(h, std::string(b) + "attn.qkv.weight", {3 * D, D}); load(h, std::string(b) + "attn.proj.weight", {D, D});
  load(h, std::string(b) + "mlp.fc1.weight", {4 * D, D}); load(h, std::string(b) + "mlp.fc2.weight", {D, 4 * D});
  const std::string p = kind != 0 ? "gpt.transformer." : "decoder.transformer.";
  if (kind == 0) { load(h, "clip_project.model.0.weight", {E, 64}); load(h, "clip_project.model.0.bias", {E}); }
  if (kind == 2) {
    load(h, "clip_project.model.0.weight", {768, 384}); load(h, "clip_project.model.0.bias", {768});
    load(h, "clip_project.model.2.weight", {2 * E, 768}); load(h, "clip_project.model.2.bias", {2 * E});
  }
  load(h, p + "wte.weight", {64, E}); load(h, p + "wpe.weight", {160, E}); load(h, p + "ln_f.weight", {E}); load(h, p + "ln_f.bias", {E});
  const std::string l = p + "h.0.";
  load(h, l + "ln_1.weight", {E}); load(h, l + "ln_1.bias", {E}); load(h, l + "ln_2.weight", {E}); load(h, l + "ln_2.bias", {E});
  load(h, l + "attn.c_attn.weight", {E, 3 * E}); load(h, l + "attn.c_attn.bias", {3 * E}); load(h, l + "attn.c_proj.weight", {E, E});
  load(h, l + "attn.c_proj.bias", {E}); load(h, l + "mlp.c_fc.weight", {E, 4 * E}); load(h, l + "mlp.c_fc.bias", {4 * E});
  load(h, l + "mlp.c_proj.weight", {4 * E, E}); load(h, l + "mlp.c_proj.bias", {E});
  if (viecap) {
    load(h, "mapping_network.linear.weight", {2 * E, 64}); load(h, "mapping_network.linear.bias", {2 * E}); load(h, "mapping_network.prefix_const", {3, E});
    const std::string m = "mapping_network.transformer.layers.0.";
    for (const char* k : {"norm1.weight", "norm1.bias", "attn.project.bias", "norm2.weight", "norm2.bias", "mlp.fc2.bias"}) load(h, m + k, {E});
    load(h, m + "attn.to_queries.weight", {E, E}); load(h, m + "attn.to_keys_values.weight", {2 * E, E}); load(h, m + "attn.project.weight", {E, E});
    load(h, m + "mlp.fc1.weight", {64, E}); load(h, m + "mlp.fc1.bias", {64}); load(h, m + "mlp.fc2.weight", {E, 64});
  }
  EXPECT_FAIL(pio_load_weight(h, "no.such.key", nullptr, nullptr, 0));
  CK(pio_finalize_weights(h));
  EXPECT_FAIL(pio_finalize_weights(h));
  return h;
}

// The CLIP ViT variant (vit_arch 1: no registers, native grid, norm_pre, bias-free patch conv, no LayerScale, head) in the
// exact-fp32 parity mode (vit_operand_type 2: fp32 weight copies and workspaces): load, finalize, forward, misuse, destroy.
static void clip_fp32_round() {
  pio_config c;
  memset(&c, 0, sizeof(c));
  c.embed_dim = 64; c.depth = 1; c.num_heads = 1; c.patch_size = 16; c.num_registers = 0; c.pretrain_grid = 2; c.crop_dim = 32;
  c.vit_ln_eps = 1e-5f; c.readout_heads = 1; c.readout_scale = 0.125f; c.dec_layers = 1; c.dec_heads = 4; c.dec_embd = 768;
  c.dec_vocab = 64; c.dec_positions = 160; c.prefix_size = 32; c.dec_ln_eps = 1e-5f; c.max_batch = 2; c.max_prefixes = 4;
  c.max_steps = 30; c.vit_operand_type = 2; c.device = 0; c.vit_arch = 1; c.vit_out_dim = 32;
  pio_handle bad = nullptr;
  pio_config w = c;
  w.num_registers = 4;
  EXPECT_FAIL(pio_create(&w, &bad));                                   // the CLIP ViT has no registers
  w = c; w.vit_arch = 0;
  EXPECT_FAIL(pio_create(&w, &bad));                                   // a head width other than embed_dim needs vit_arch 1
  pio_handle h = nullptr;
  CK(pio_create(&c, &h));
  const int64_t D = 64;
  load(h, "cls_token", {1, 1, D}); load(h, "pos_embed", {1, 5, D}); load(h, "patch_embed.proj.weight", {D, 3, 16, 16});
  load(h, "norm.weight", {D}); load(h, "norm.bias", {D}); load(h, "norm_pre.weight", {D}); load(h, "norm_pre.bias", {D});
  load(h, "head.weight", {32, D});
  const char* b = "blocks.0.";
  for (const char* k : {"norm1.weight", "norm1.bias", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc2.bias"}) load(h, std::string(b) + k, {D});
  load(h, std::string(b) + "attn.qkv.bias", {3 * D}); load(h, std::string(b) + "mlp.fc1.bias", {4 * D});
  load(h, std::string(b) + "attn.qkv.weight", {3 * D, D}); load(h, std::string(b) + "attn.proj.weight", {D, D});
  load(h, std::string(b) + "mlp.fc1.weight", {4 * D, D}); load(h, std::string(b) + "mlp.fc2.weight", {D, 4 * D});
  CK(pio_finalize_weights(h));
  std::vector<float> imgs(2 * 3 * 32 * 32, 0.1f), tok(2 * 5 * 32), qkv(2 * 5 * 192), sa(2 * 4);
  CK(pio_vit_forward(h, imgs.data(), 2, tok.data(), nullptr, nullptr));
  EXPECT_FAIL(pio_vit_forward(h, imgs.data(), 2, tok.data(), qkv.data(), nullptr));          // no qkv capture on this backbone
  EXPECT_FAIL(pio_cls_attention(h, qkv.data(), tok.data(), 2, sa.data(), nullptr, nullptr, nullptr, nullptr));
  CK(pio_destroy(h));
}

// The AlphaCLIP ViT (vit_arch 2: four-channel patch rows, masks) and the RegionCLIP ResNet tower (vit_arch 3: the handle owns the RnNet
// that rn_build hands out): create, load, finalize, forward, misuse, destroy.
static void alpha_and_resnet_round() {
  pio_config c;
  memset(&c, 0, sizeof(c));
  c.embed_dim = 64; c.depth = 1; c.num_heads = 1; c.patch_size = 16; c.num_registers = 0; c.pretrain_grid = 2; c.crop_dim = 32;
  c.vit_ln_eps = 1e-5f; c.readout_heads = 1; c.readout_scale = 0.125f; c.dec_layers = 1; c.dec_heads = 4; c.dec_embd = 768;
  c.dec_vocab = 64; c.dec_positions = 160; c.prefix_size = 64; c.dec_ln_eps = 1e-5f; c.max_batch = 3; c.max_prefixes = 4;
  c.max_steps = 30; c.vit_operand_type = 0; c.device = 0; c.vit_arch = 2;
  pio_handle h = nullptr;
  CK(pio_create(&c, &h));
  const int64_t D = 64;
  load(h, "cls_token", {1, 1, D}); load(h, "pos_embed", {1, 5, D}); load(h, "patch_embed.proj.weight", {D, 3, 16, 16});
  load(h, "patch_embed.alpha.weight", {D, 1, 16, 16});
  load(h, "norm.weight", {D}); load(h, "norm.bias", {D}); load(h, "norm_pre.weight", {D}); load(h, "norm_pre.bias", {D});
  const char* b = "blocks.0.";
  for (const char* k : {"norm1.weight", "norm1.bias", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc2.bias"}) load(h, std::string(b) + k, {D});
  load(h, std::string(b) + "attn.qkv.bias", {3 * D}); load(h, std::string(b) + "mlp.fc1.bias", {4 * D});
  load(h, std::string(b) + "attn.qkv.weight", {3 * D, D}); load(h, std::string(b) + "attn.proj.weight", {D, D});
  load(h, std::string(b) + "mlp.fc1.weight", {4 * D, D}); load(h, std::string(b) + "mlp.fc2.weight", {D, 4 * D});
  CK(pio_finalize_weights(h));
  std::vector<float> imgs(2 * 3 * 32 * 32, 0.1f), tok(3 * 5 * 64), boxes(3 * 4, 0.25f);
  std::vector<int32_t> img_of{0, 1, 1}, box_off{0, 1, 2, 2}, pt_off{0, 0, 0, 2};
  std::vector<double> pts{0.1, 0.2, 0.3, 0.4};
  std::vector<uint8_t> masks(3 * 32 * 32, 1);
  CK(pio_region_masks(h, boxes.data(), box_off.data(), pts.data(), pt_off.data(), 3, 32, 1.f, masks.data(), nullptr));
  EXPECT_FAIL(pio_region_masks(h, boxes.data(), box_off.data(), pts.data(), pt_off.data(), 3, 0, 1.f, masks.data(), nullptr));
  CK(pio_vit_forward_regions(h, imgs.data(), img_of.data(), masks.data(), 3, tok.data(), nullptr));
  CK(pio_vit_forward_regions(h, imgs.data(), nullptr, nullptr, 2, tok.data(), nullptr));
  EXPECT_FAIL(pio_vit_forward_regions(h, imgs.data(), img_of.data(), masks.data(), 4, tok.data(), nullptr));     // above max_batch
  CK(pio_vit_forward(h, imgs.data(), 2, tok.data(), nullptr, nullptr));
  CK(pio_destroy(h));

  c.vit_arch = 3; c.embed_dim = 512; c.num_heads = 8; c.patch_size = 32; c.crop_dim = 64; c.readout_heads = 8; c.rn_width = 16;
  for (int i = 0; i < 4; ++i) c.rn_layers[i] = 1;
  c.max_batch = 2;
  pio_handle bad = nullptr;
  pio_config w = c;
  w.rn_width = 12;
  EXPECT_FAIL(pio_create(&w, &bad));                                   // the width must be a multiple of 16
  // a handle that never got the tower (nothing to destroy), and one that owns it
  CK(pio_create(&c, &h));
  CK(pio_destroy(h));
  CK(pio_create(&c, &h));
  load(h, "rn.conv1.weight", {8, 3, 3, 3});
  CK(pio_finalize_weights(h));
  std::vector<float> rimgs(2 * 3 * 64 * 64, 0.1f), rtok(2 * 5 * 512);
  CK(pio_vit_forward(h, rimgs.data(), 2, rtok.data(), nullptr, nullptr));
  EXPECT_FAIL(pio_vit_forward(h, rimgs.data(), 3, rtok.data(), nullptr, nullptr));
  CK(pio_destroy(h));
}

// The sparse last block and the compact-row reduction on a DINOv2 handle (max_batch 2, Tp 16).
static void drive_rows(pio_handle h) {
  std::vector<float> imgs(2 * 3 * 28 * 28), tok(8 * 64), wts(3 * 4, 0.25f), out(3 * 64);
  std::vector<int32_t> quads{4, 16}, off{0, 1, 2}, row_map(2 * 4), img_index{0, 1, 1};
  CK(pio_vit_forward_rows(h, imgs.data(), 2, quads.data(), off.data(), tok.data(), row_map.data(), nullptr));
  if (row_map[0] != -1 || row_map[7] != -1) { printf("row_map not reset\n"); exit(4); }
  CK(pio_region_reduce_rows(h, tok.data(), row_map.data(), wts.data(), img_index.data(), 3, 1.f, out.data(), nullptr));
  CK(pio_region_reduce_rows(h, tok.data(), row_map.data(), wts.data(), nullptr, 2, 1.f, out.data(), nullptr));
  std::vector<int32_t> unsorted{16, 4};
  EXPECT_FAIL(pio_vit_forward_rows(h, imgs.data(), 2, unsorted.data(), off.data(), tok.data(), row_map.data(), nullptr));
  std::vector<int32_t> many{0, 4, 8, 16, 20, 24}, many_off{0, 3, 6};                     // 24 of 32 rows: above the share the sparse block takes
  EXPECT_FAIL(pio_vit_forward_rows(h, imgs.data(), 2, many.data(), many_off.data(), tok.data(), row_map.data(), nullptr));
  EXPECT_FAIL(pio_region_reduce_rows(h, tok.data(), row_map.data(), wts.data(), img_index.data(), 0, 1.f, out.data(), nullptr));
}

// The prompted cache (12 graphs) of a language-model handle with max_prefixes 4 past its capacity, the four kinds mixed: 15 keys, the first
// launched on a stream that is destroyed before its entry is evicted, then the first again (recaptured) and the last (resident); one failed
// instantiate and one failed event creation on keys of their own.  map: the handle (or for a clone its owner) has a mapping network, whose
// soft prompt is 3 positions; own_map: the handle itself has it.  P + steps - 1 stays inside 30 positions, the smallest max_steps here.
static void drive_prompted(pio_handle d, bool map, bool own_map) {
  const int E = 768, V = 64;
  std::vector<float> cont(4 * 3 * E, 0.1f), embeds(4 * 8 * E, 0.1f), scores(4), unif(4 * 8, 0.5f), logits((size_t)4 * V, 0.f);
  std::vector<int32_t> toks(4 * 8, 1), tl{8, 1, 0, 5}, plen{5, 8, 3, 8}, ids(4 * 8), lens(4), active(4, 1), kept(4);
  const float* soft = own_map ? cont.data() : nullptr;          // pio_viecap_decode reads the handle's own mapping network
  const float* rsoft = map ? cont.data() : nullptr;             // the ragged entry points read the owner's
  void* s1 = nullptr;
  CK(pio_stream_create(0, 0, 192, &s1));
  CK(pio_viecap_decode(d, soft, toks.data(), 2, 1, 1, 8, ids.data(), s1));                                    // key 1, on s1
  CK(pio_stream_destroy(s1));
  for (int Lt = 2; Lt <= 5; ++Lt) CK(pio_viecap_decode(d, soft, toks.data(), 2, Lt, 1, 8, ids.data(), nullptr));     // 2 .. 5
  for (int N = 1; N <= 4; ++N) CK(pio_viecap_decode_ragged(d, rsoft, toks.data(), tl.data(), N, 8, 1, 8, ids.data(), nullptr));     // 6 .. 9
  CK(pio_viecap_decode_ragged(d, nullptr, toks.data(), tl.data(), 4, 8, 0, 8, ids.data(), nullptr));         // hard prompt only: same key as N = 4 only without a soft prompt
  EXPECT_FAIL(pio_viecap_decode_ragged(d, nullptr, nullptr, nullptr, 2, 0, 1, 8, ids.data(), nullptr));      // neither kind of prompt
  EXPECT_FAIL(pio_viecap_decode_ragged(d, rsoft, toks.data(), tl.data(), 5, 8, 1, 8, ids.data(), nullptr));  // above max_prefixes
  CK(pio_lm_beam_search(d, embeds.data(), nullptr, 2, 8, 2, 6, 1, 2, ids.data(), lens.data(), scores.data(), nullptr));     // 10 (or 11 with the hard-only ragged key)
  CK(pio_lm_beam_search(d, embeds.data(), plen.data(), 2, 8, 2, 6, 1, 2, ids.data(), lens.data(), scores.data(), nullptr));
  CK(pio_lm_beam_search(d, embeds.data(), plen.data(), 1, 8, 4, 6, 1, 2, ids.data(), lens.data(), scores.data(), nullptr));
  EXPECT_FAIL(pio_lm_beam_search(d, embeds.data(), plen.data(), 2, 8, 3, 6, 1, 2, ids.data(), lens.data(), scores.data(), nullptr));   // 6 rows
  EXPECT_FAIL(pio_lm_beam_search(d, embeds.data(), plen.data(), 2, 8, 2, 6, 1, 64, ids.data(), lens.data(), scores.data(), nullptr));  // eos outside the vocabulary
  CK(pio_lm_sample(d, embeds.data(), 3, 8, 8, 1.f, 0.8f, 1, 0, unif.data(), ids.data(), lens.data(), nullptr));       // given uniforms
  CK(pio_lm_sample(d, embeds.data(), 3, 8, 8, 1.f, 0.8f, 1, 1234, nullptr, ids.data(), lens.data(), nullptr));        // a seed: the same key
  CK(pio_lm_sample(d, embeds.data(), 3, 8, 8, 0.7f, 0.8f, 1, 1234, nullptr, ids.data(), lens.data(), nullptr));       // another temperature: another graph
  CK(pio_lm_sample(d, embeds.data(), 3, 8, 8, 0.7f, 0.9f, 2, 1234, nullptr, ids.data(), lens.data(), nullptr));       // 15 or more keys by now
  EXPECT_FAIL(pio_lm_sample(d, embeds.data(), 5, 8, 8, 1.f, 0.8f, 1, 0, unif.data(), ids.data(), lens.data(), nullptr));
  EXPECT_FAIL(pio_lm_sample(d, embeds.data(), 3, 8, 8, 1.f, 0.8f, 64, 0, unif.data(), ids.data(), lens.data(), nullptr));
  CK(pio_viecap_decode(d, soft, toks.data(), 2, 1, 1, 8, ids.data(), nullptr));                              // key 1 again: evicted behind its dead stream, recaptured
  CK(pio_lm_sample(d, embeds.data(), 3, 8, 8, 0.7f, 0.9f, 2, 7, nullptr, ids.data(), lens.data(), nullptr)); // the last key: resident
  // a failed instantiate leaves an entry without an exec, which the same call then captures; a failed event creation leaves no entry
  hip_stub_fail_next_graph_instantiate();
  EXPECT_HIP(pio_viecap_decode(d, soft, toks.data(), 3, 2, 1, 8, ids.data(), nullptr));
  CK(pio_viecap_decode(d, soft, toks.data(), 3, 2, 1, 8, ids.data(), nullptr));
  hip_stub_fail_next_event_create();
  EXPECT_HIP(pio_lm_beam_search(d, embeds.data(), nullptr, 1, 8, 2, 6, 1, 2, ids.data(), lens.data(), scores.data(), nullptr));
  CK(pio_lm_beam_search(d, embeds.data(), nullptr, 1, 8, 2, 6, 1, 2, ids.data(), lens.data(), scores.data(), nullptr));
  CK(pio_nucleus_sample(d, logits.data(), 4, 1.f, 0.8f, unif.data(), 1, active.data(), ids.data(), kept.data(), nullptr));
  CK(pio_nucleus_sample(d, logits.data(), 4, 1.f, 0.8f, unif.data(), 1, active.data(), ids.data(), nullptr, nullptr));
  EXPECT_FAIL(pio_nucleus_sample(d, logits.data(), 0, 1.f, 0.8f, unif.data(), 1, active.data(), ids.data(), nullptr, nullptr));
}

// The stop cache (8 decodes) past its capacity: 11 decodes of 8 steps in segments of 2 or 3, those whose stop id is 0 ended by the stub's scan
// after their first segment and the others run to their last; the first on a stream that is destroyed before its eviction, then the first
// again; one failed instantiate in the middle of a decode and one failed event creation.  clip: the handle decodes from CLIP prefixes
// (pio_decode_greedy_stop), else from prompts (pio_viecap_decode_stop; a clone has no mapping network and takes hard prompts only).
static void drive_stop(pio_handle d, bool clip, bool own_map) {
  std::vector<float> prefix(4 * 64, 0.1f), cont(4 * 3 * 768, 0.1f);
  std::vector<int32_t> toks(4 * 8, 1), ids(4 * 8);
  const float* soft = own_map ? cont.data() : nullptr;
  int32_t ran = -1;
  auto decode = [&](int N, int eos, int seg, void* s) {
    return clip ? pio_decode_greedy_stop(d, prefix.data(), N, 8, eos, seg, ids.data(), &ran, s)
                : pio_viecap_decode_stop(d, soft, toks.data(), N, 4, 1, 8, eos, -1, seg, ids.data(), &ran, s);
  };
  auto expect_ran = [&](int want) { if (ran != want) { printf("steps_run %d, expected %d\n", ran, want); exit(4); } };
  void* s1 = nullptr;
  CK(pio_stream_create(0, 0, 192, &s1));
  CK(decode(1, 0, 2, s1)); expect_ran(2);                          // decode 1, ended early, on s1
  CK(pio_stream_destroy(s1));
  for (int N = 1; N <= 4; ++N) { CK(decode(N, 5, 2, nullptr)); expect_ran(8); }       // 2 .. 5: all four segments
  for (int N = 2; N <= 4; ++N) { CK(decode(N, 0, 3, nullptr)); expect_ran(3); }       // 6 .. 8: ended after the first of three
  CK(decode(2, 0, 3, nullptr)); expect_ran(3);                     // replay: the stub's scan does not run, the count of the last decode stands
  CK(decode(1, 5, 3, nullptr)); expect_ran(8);                     // 9: the cache is full, decode 1 goes (its stream is gone)
  CK(decode(2, 5, 3, nullptr)); expect_ran(8);                     // 10
  CK(decode(1, 5, 8, nullptr)); expect_ran(8);                     // 11: one segment, nothing to wait for
  CK(decode(1, 5, 64, nullptr)); expect_ran(8);                    // seg above steps: the same key
  CK(decode(1, 0, 2, nullptr)); expect_ran(2);                     // decode 1 again: recaptured
  hip_stub_fail_next_graph_instantiate();
  EXPECT_HIP(decode(3, 6, 2, nullptr));                            // a new decode whose first segment fails to instantiate ...
  CK(decode(3, 6, 2, nullptr)); expect_ran(8);                     // ... and is captured by the next call
  hip_stub_fail_next_event_create();
  EXPECT_HIP(decode(3, 7, 2, nullptr));
  CK(decode(3, 7, 2, nullptr)); expect_ran(8);
  EXPECT_FAIL(decode(5, 5, 2, nullptr));                           // above max_prefixes
  EXPECT_FAIL(decode(2, 5, 0, nullptr));                           // seg < 1
  EXPECT_FAIL(decode(2, -1, 2, nullptr));                          // no stop id
}

int main() {
  for (int it = 0; it < 12; ++it) {
    if (it < 3) { clip_fp32_round(); alpha_and_resnet_round(); }
    pio_handle h = make(false);
    std::vector<float> bank(16 * 384, 0.5f);
    for (int d = 0; d < 384; ++d) bank[5 * 384 + d] = 0.f;             // one zero row: dropped at load
    int64_t kept = 0;
    CK(pio_set_memory_bank(h, bank.data(), 16, 384, &kept));
    if (kept != 15) { printf("kept %lld\n", (long long)kept); return 4; }
    EXPECT_FAIL(pio_set_memory_bank(h, bank.data(), 16, 384, &kept));   // already set
    pio_handle c1 = nullptr, c2 = nullptr, bad = nullptr;
    CK(pio_clone_decoder(h, &c1));
    CK(pio_clone_decoder(h, &c2));
    EXPECT_FAIL(pio_clone_decoder(c1, &bad));                            // clones of clones are refused
    EXPECT_FAIL(pio_destroy(h));                                         // the owner outlives its clones
    std::vector<float> prefix(4 * 64, 0.1f), tok(2 * 9 * 64), qkv(2 * 9 * 192);
    std::vector<int32_t> ids(4 * 30);
    std::vector<float> lp(4 * 30), imgs(2 * 3 * 28 * 28);
    for (pio_handle d : {h, c1, c2}) {
      CK(pio_decode_greedy(d, prefix.data(), 3, 30, ids.data(), nullptr, nullptr));
      CK(pio_decode_greedy(d, prefix.data(), 4, 30, ids.data(), lp.data(), nullptr));     // a second graph key
      CK(pio_decode_greedy(d, prefix.data(), 3, 30, ids.data(), nullptr, nullptr));     // replay
      EXPECT_FAIL(pio_decode_greedy(d, prefix.data(), 5, 30, ids.data(), nullptr, nullptr));
    }
    CK(pio_vit_forward(h, imgs.data(), 2, tok.data(), qkv.data(), nullptr));
    CK(pio_profile_enable(h, 1));
    CK(pio_vit_forward(h, imgs.data(), 1, tok.data(), nullptr, nullptr));
    double ms, fl, by; int64_t n;
    CK(pio_profile_read(h, 0, &ms, &n, &fl, &by));
    CK(pio_profile_enable(h, 0));
    void* s1 = nullptr; void* s2 = nullptr;
    CK(pio_stream_create(0, 0, 192, &s1));
    CK(pio_stream_create(0, 192, 64, &s2));
    CK(pio_decode_greedy(c1, prefix.data(), 2, 30, ids.data(), nullptr, s1));
    CK(pio_stream_destroy(s1));
    CK(pio_stream_destroy(s2));
    // the sparse last block; then all three graph caches of the owner and of a clone populated and driven past their bounds before teardown
    drive_rows(h);
    for (pio_handle d : {h, c2}) {
      drive_stop(d, true, false);
      drive_prompted(d, false, false);
    }
    hip_stub_fail_next_graph_instantiate();
    EXPECT_HIP(pio_decode_greedy(c1, prefix.data(), 1, 30, ids.data(), nullptr, nullptr));     // the unbounded cache: an entry without an exec ...
    CK(pio_decode_greedy(c1, prefix.data(), 1, 30, ids.data(), nullptr, nullptr));             // ... captured by the next call
    // teardown in the order that matters: clones (either order), then the owner
    if (it & 1) { CK(pio_destroy(c1)); CK(pio_destroy(c2)); } else { CK(pio_destroy(c2)); CK(pio_destroy(c1)); }
    CK(pio_destroy(h));
    // ViECap head: mapping network + entity table + prompted decode graphs
    pio_handle v = make(true);
    std::vector<float> ent(5 * 64, 0.3f), feats(4 * 64, 0.2f), cont(4 * 3 * 768), probs(4 * 5);
    std::vector<int32_t> toks(4 * 6, 1), vids(4 * 64);
    CK(pio_viecap_set_entities(v, ent.data(), 5, 64));
    EXPECT_FAIL(pio_viecap_set_entities(v, ent.data(), 5, 64));
    CK(pio_viecap_mapping(v, feats.data(), 4, cont.data(), nullptr));
    CK(pio_viecap_entity_logits(v, feats.data(), 4, 0.01f, probs.data(), nullptr));
    CK(pio_viecap_decode(v, cont.data(), toks.data(), 4, 6, 1, 64, vids.data(), nullptr));
    CK(pio_viecap_decode(v, cont.data(), toks.data(), 2, 4, 1, 64, vids.data(), nullptr));
    CK(pio_viecap_decode(v, cont.data(), nullptr, 2, 0, 1, 64, vids.data(), nullptr));
    EXPECT_FAIL(pio_viecap_decode(v, cont.data(), toks.data(), 4, 100, 1, 64, vids.data(), nullptr));   // positions above max_steps
    CK(pio_viecap_decode(v, nullptr, toks.data(), 2, 4, 0, 64, vids.data(), nullptr));                  // only_hard_prompt
    EXPECT_FAIL(pio_viecap_decode(v, nullptr, nullptr, 2, 0, 1, 64, vids.data(), nullptr));             // neither kind of prompt
    // beam search building blocks: prompt assembly, prefill, re-ordered advance, selection
    {
      const int vocab = 64;                       // dec_vocab of this configuration; max_prefixes = 4 beams
      std::vector<float> prompt(4 * 9 * 768), logp((size_t)4 * vocab), sc(4, -1.f), ln(4, 1.f), val(4);
      std::vector<int32_t> nt(4, 7), src{0, 0, 1, 3}, st(4, 0);
      std::vector<int64_t> idx(4);
      CK(pio_viecap_build_prompt(v, cont.data(), toks.data(), 4, 6, 1, prompt.data(), nullptr));
      CK(pio_viecap_build_prompt(v, nullptr, toks.data(), 4, 6, 0, prompt.data(), nullptr));
      EXPECT_FAIL(pio_viecap_build_prompt(v, nullptr, nullptr, 4, 0, 0, prompt.data(), nullptr));
      CK(pio_lm_prefill(v, prompt.data(), 4, 9, logp.data(), nullptr));
      CK(pio_beam_select(v, logp.data(), nullptr, nullptr, nullptr, 4, val.data(), idx.data(), nullptr));
      CK(pio_lm_advance(v, nt.data(), nullptr, 4, 9, logp.data(), nullptr));
      CK(pio_lm_advance(v, nt.data(), src.data(), 4, 10, logp.data(), nullptr));
      CK(pio_beam_select(v, logp.data(), sc.data(), ln.data(), st.data(), 4, val.data(), idx.data(), nullptr));
      EXPECT_FAIL(pio_beam_select(v, logp.data(), sc.data(), nullptr, st.data(), 4, val.data(), idx.data(), nullptr));
      EXPECT_FAIL(pio_beam_select(v, logp.data(), nullptr, nullptr, nullptr, 9, val.data(), idx.data(), nullptr));
      EXPECT_FAIL(pio_lm_prefill(v, prompt.data(), 5, 9, logp.data(), nullptr));        // above max_prefixes
      EXPECT_FAIL(pio_lm_advance(v, nt.data(), nullptr, 4, 4096, logp.data(), nullptr));
    }
    EXPECT_FAIL(pio_decode_greedy(v, prefix.data(), 2, 30, ids.data(), nullptr, nullptr));             // no clip_project in a ViECap model
    EXPECT_FAIL(pio_decode_greedy_stop(v, prefix.data(), 2, 30, 5, 2, ids.data(), vids.data(), nullptr));
    // the device hard prompt, the ragged prompt, and both bounded caches of the owner and of a clone past their capacity
    {
      std::vector<int32_t> frag_ids(12, 3), frag_off{0, 2, 4, 6, 8}, frag_len{2, 2, 2, 2, 2}, seg{0, 4}, ctok(4 * 8), clen(4), scratch(4), plen(4);
      std::vector<float> rprompt(4 * 11 * 768);
      CK(pio_viecap_compose_prompts(v, probs.data(), 4, 5, frag_ids.data(), frag_off.data(), frag_len.data(), 10, 1, 11, 1, 3, 0.2f, 0,
                                    seg.data(), 8, ctok.data(), clen.data(), scratch.data(), nullptr));
      EXPECT_FAIL(pio_viecap_compose_prompts(v, probs.data(), 4, 5, frag_ids.data(), frag_off.data(), frag_len.data(), 10, 1, 11, 1, 9, 0.2f, 0,
                                             seg.data(), 8, ctok.data(), clen.data(), scratch.data(), nullptr));     // top_k above 8
      pio_handle vc = nullptr;
      CK(pio_clone_decoder(v, &vc));
      for (pio_handle d : {v, vc}) {
        CK(pio_viecap_build_prompt_ragged(d, cont.data(), toks.data(), clen.data(), 4, 6, 1, rprompt.data(), plen.data(), nullptr));
        CK(pio_viecap_build_prompt_ragged(d, nullptr, toks.data(), clen.data(), 4, 6, 0, rprompt.data(), plen.data(), nullptr));
        EXPECT_FAIL(pio_viecap_build_prompt_ragged(d, nullptr, nullptr, nullptr, 4, 0, 0, rprompt.data(), plen.data(), nullptr));
        drive_prompted(d, true, d == v);
        drive_stop(d, false, d == v);
      }
      if (it & 1) { CK(pio_destroy(vc)); CK(pio_destroy(v)); }
      else { EXPECT_FAIL(pio_destroy(v)); CK(pio_destroy(vc)); CK(pio_destroy(v)); }
    }
    // ClipCap head: the MLP prefix mapper, then sampling from its prefixes
    if (it < 3) {
      pio_handle k = make(2);
      std::vector<float> cf(4 * 384, 0.2f), pre(4 * 2 * 768);
      if (pio_clipcap_prefix_length(k) != 2) { printf("prefix length %d\n", pio_clipcap_prefix_length(k)); return 4; }
      CK(pio_clipcap_mapping(k, cf.data(), 4, 1, pre.data(), nullptr));
      CK(pio_clipcap_mapping(k, cf.data(), 2, 0, pre.data(), nullptr));
      EXPECT_FAIL(pio_clipcap_mapping(k, cf.data(), 5, 1, pre.data(), nullptr));
      EXPECT_FAIL(pio_clipcap_mapping(nullptr, cf.data(), 2, 0, pre.data(), nullptr));
      std::vector<int32_t> sid(4 * 8), slen(4);
      CK(pio_lm_sample(k, pre.data(), 4, 2, 8, 1.f, 0.8f, 1, 42, nullptr, sid.data(), slen.data(), nullptr));
      CK(pio_destroy(k));
    }
  }
  CK(pio_destroy(nullptr));
  printf("asan loop ok\n");
  return 0;
}
