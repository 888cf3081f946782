"""Float reference of the INViTE backbone path (P/src/INViTE/clipfolder/model.py:171-284; P/src/model.py:818-827), for the INViTE tests
and tools/oracle/gen_golden_invite.py.  No test functions here.

* the tower is OpenAI's CLIP ViT: patch convolution without bias, class embedding, learned positions, ln_pre, pre-LN blocks with
  QuickGELU, then ln_post and the bias-free projection on EVERY token (get_all_last);
* its last k blocks (extract_last_k_th_token) carry an attention mask that is -inf off the diagonal.  Every softmax row is then exactly
  1 on itself, so such a block is stated here as what it computes: x += out_proj(W_v ln_1(x) + b_v), then the MLP.  ``masked_block_attention``
  is the same branch THROUGH the mask and softmax, kept for the test that the two are the same bits;
* ``dtype`` float32 is the arithmetic of the reference on the CPU, float64 the yardstick the fp32 bars are measured against;
* the captioning driver is ``oracle.patchioner_oracle.PatchionerOracle``: the tower is one ordinary forward, so boxes, traces and the
  decoder run as they do behind the CLIP backbone.

Weights are the ENGINE's keys (weights.invite_to_engine): fp16-rounded where the reference's loader rounds, the position table already
at the tower's grid."""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn.functional as F

from oracle import patchioner_oracle as O

# ---- inputs shared by the fixture generator and the tests ------------------------------------------------------------------
CASE = dict(depth=3, seed_vit=131, seed_text=133, seed_dec=137, seed_bank=143, seed_img=101, bank_rows=2048, B=2)
# tower cases of tests/golden/invite.npz: name, invite_config resolution (None: native), extract_last_k_th_token, crop, and the stride
# of the token rows the fixture keeps (row 0, the CLS token, is always among them)
TOWERS = {
    "b16_k1": dict(name="ViT-B/16", resolution=None, k=1, crop=224, stride=8),
    "b16_r288_k1": dict(name="ViT-B/16", resolution=288, k=1, crop=288, stride=12),
    "b32_k2": dict(name="ViT-B/32", resolution=None, k=2, crop=224, stride=2),
    "b16_km1": dict(name="ViT-B/16", resolution=None, k=-1, crop=224, stride=8),
}
FORWARD_TOWERS = ("b16_k1", "b32_k2")            # the towers whose Patchioner.forward ids and strings the fixture records
POS_SAMPLE = (slice(None, None, 9), slice(None, None, 16))      # the sample of the resampled position table (b16_r288_k1)
# max |reference fp32 tokens - float64 tower| / max |reference| per case, measured on the CPU (tests/test_invite_cpu.py re-measures it
# and holds the record); the fp32 parity mode of the engine is held to four times it (tests/test_gpu_invite.py)
REF_FP32_VS_F64 = {"b16_k1": 6.58e-7, "b16_r288_k1": 9.36e-7, "b32_k2": 1.11e-6, "b16_km1": 6.66e-7}


def self_only_layers(k: int, depth: int) -> int:
    """clipfolder/model.py:216-217: k <= 0 masks nothing, k >= layers masks every block."""
    return 0 if k <= 0 else min(k, depth)


def boxes(crop: int) -> torch.Tensor:
    """[B, 4, 4] xywh boxes in crop pixels (scaled from a 224 crop), one dummy (all -1) per image."""
    b = torch.tensor([[[10.0, 20.0, 60.0, 50.0], [100.5, 30.25, 80.0, 120.75], [-1.0, -1.0, -1.0, -1.0], [150.0, 150.0, 70.0, 70.0]],
                      [[40.0, 40.0, 32.0, 48.0], [-1.0, -1.0, -1.0, -1.0], [5.0, 150.0, 200.0, 60.0], [64.0, 0.0, 96.0, 224.0]]])
    return torch.where(b < 0, b, b * (crop / 224.0))


def traces() -> List[List[dict]]:
    return [[{"x": 0.2 + 0.02 * i, "y": 0.3 + 0.015 * i} for i in range(25)],
            [{"x": 0.7 - 0.01 * i, "y": 0.6 + 0.012 * (i % 7)} for i in range(30)]]


FORWARD_CASES = [("cls", dict(get_cls_capt=True)),
                 ("boxes", dict(get_cls_capt=False, bboxes=True, gaussian_avg=True, gaussian_bbox_variance=0.5)),
                 ("traces", dict(get_cls_capt=False, traces=True))]


def forward_args(kw: dict, crop: int) -> dict:
    kw = dict(kw)
    if kw.get("bboxes"):
        kw["bboxes"] = boxes(crop)
    if kw.get("traces"):
        kw["traces"] = traces()
    return kw


# ---- the tower -------------------------------------------------------------------------------------------------------------
class InviteViTOracle:
    """INViTE's VisionTransformer over engine-layout weights, with the interface PatchionerOracle expects of a backbone."""

    has_attention = False          # P/src/model.py:864-865: no qkv hook on this backbone
    R = 0

    def __init__(self, w: Dict[str, torch.Tensor], num_heads: int, patch_size: int, self_only: int, dtype=torch.float32,
                 eps: float = 1e-5):
        self.w = {k: v.detach().cpu().to(dtype) for k, v in w.items()}
        self.num_heads, self.patch_size, self.eps, self.dtype = num_heads, patch_size, eps, dtype
        self.depth = 1 + max(int(k.split(".")[1]) for k in self.w if k.startswith("blocks."))
        self.self_only = self_only
        self.Dv = self.w["cls_token"].shape[-1]
        self.D = self.w["head.weight"].shape[0]
        self.last_qkv = None

    def _ln(self, x, key):
        return F.layer_norm(x, (self.Dv,), self.w[key + ".weight"], self.w[key + ".bias"], self.eps)

    def attention(self, i: int, y: torch.Tensor) -> torch.Tensor:
        """The attention branch of block i on y = ln_1(x) [B, T, D], before out_proj."""
        w, D, h = self.w, self.Dv, self.num_heads
        pre = "blocks.%d." % i
        if i >= self.depth - self.self_only:        # the diagonal mask: every token attends to itself, its output is its own V row
            return F.linear(y, w[pre + "attn.qkv.weight"][2 * D:], w[pre + "attn.qkv.bias"][2 * D:])
        B, T = y.shape[:2]
        q, k, v = F.linear(y, w[pre + "attn.qkv.weight"], w[pre + "attn.qkv.bias"]).reshape(B, T, 3, h, D // h).permute(2, 0, 3, 1, 4)
        a = ((q * (D // h) ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
        return (a @ v).transpose(1, 2).reshape(B, T, D)

    def masked_block_attention(self, i: int, s: torch.Tensor) -> torch.Tensor:
        """The attention branch of block i, out_proj included, through torch.nn.MultiheadAttention with the reference's mask (-inf off
        the diagonal, 0 on it), as ResidualAttentionBlock.attention runs it: s = ln_1(x) SEQUENCE-FIRST [T, B, D], need_weights=False."""
        w, D = self.w, self.Dv
        pre = "blocks.%d." % i
        T = s.shape[0]
        mha = torch.nn.MultiheadAttention(D, self.num_heads).to(self.dtype).eval()
        mha.load_state_dict({"in_proj_weight": w[pre + "attn.qkv.weight"], "in_proj_bias": w[pre + "attn.qkv.bias"],
                             "out_proj.weight": w[pre + "attn.proj.weight"], "out_proj.bias": w[pre + "attn.proj.bias"]})
        mask = torch.full((T, T), float("-inf"), dtype=self.dtype)
        mask.fill_diagonal_(0)
        return mha(s, s, s, need_weights=False, attn_mask=mask)[0]

    def v_only_attention(self, i: int, s: torch.Tensor) -> torch.Tensor:
        """What the masked branch computes, in the same layout: out_proj(W_v s + b_v), nothing of q or k."""
        w, D = self.w, self.Dv
        pre = "blocks.%d." % i
        v = F.linear(s, w[pre + "attn.qkv.weight"][2 * D:], w[pre + "attn.qkv.bias"][2 * D:])
        return F.linear(v, w[pre + "attn.proj.weight"], w[pre + "attn.proj.bias"])

    def embed(self, imgs: torch.Tensor) -> torch.Tensor:
        w, D = self.w, self.Dv
        B = imgs.shape[0]
        x = F.conv2d(imgs.to(self.dtype), w["patch_embed.proj.weight"], None, stride=self.patch_size).flatten(2).transpose(1, 2)
        x = torch.cat([w["cls_token"].reshape(1, 1, D).expand(B, -1, -1), x], dim=1)
        pos = w["pos_embed"].reshape(1, -1, D)
        if pos.shape[1] != x.shape[1]:
            raise RuntimeError("The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1"
                               % (x.shape[1], pos.shape[1]))
        return self._ln(x + pos, "norm_pre")

    def tokens(self, imgs: torch.Tensor) -> torch.Tensor:
        """[B, 1 + n^2, output_dim]: every token through ln_post and proj (get_all_last)."""
        w = self.w
        x = self.embed(imgs)
        for i in range(self.depth):
            pre = "blocks.%d." % i
            x = x + F.linear(self.attention(i, self._ln(x, pre + "norm1")), w[pre + "attn.proj.weight"], w[pre + "attn.proj.bias"])
            y = F.linear(self._ln(x, pre + "norm2"), w[pre + "mlp.fc1.weight"], w[pre + "mlp.fc1.bias"])
            y = y * torch.sigmoid(1.702 * y)
            x = x + F.linear(y, w[pre + "mlp.fc2.weight"], w[pre + "mlp.fc2.bias"])
        return F.linear(self._ln(x, "norm"), w["head.weight"])

    def __call__(self, imgs: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = self.tokens(imgs)
        return {"x_norm_clstoken": out[:, 0], "x_norm_regtokens": out[:, 1:1], "x_norm_patchtokens": out[:, 1:]}


def tower_weights(tag: str, depth: int = None) -> Dict[str, torch.Tensor]:
    """The engine-layout weights of tower case ``tag``: the seeded synthetic checkpoint through the loader's rules."""
    from patchioner_amd import weights as W
    t = TOWERS[tag]
    return W.invite_to_engine(W.synth_invite_vit(CASE["seed_vit"], t["name"], depth=depth or CASE["depth"]), resolution=t["resolution"])


def tower(tag: str, dtype=torch.float32) -> InviteViTOracle:
    from patchioner_amd import weights as W
    t = TOWERS[tag]
    _, _, heads, patch, _, _ = W.invite_arch(t["name"])
    return InviteViTOracle(tower_weights(tag), heads, patch, self_only_layers(t["k"], CASE["depth"]), dtype=dtype)


def images(tag: str) -> torch.Tensor:
    from patchioner_amd import weights as W
    return W.synth_images(CASE["seed_img"], CASE["B"], TOWERS[tag]["crop"])


def driver(tag: str):
    """(PatchionerOracle over the float tower, DeCapOracle) with the seeded decoder and bank of the forward cases."""
    from patchioner_amd import weights as W
    from patchioner_amd.tokenizer import ClipDetokenizer
    bank = W.synth_bank(CASE["seed_bank"], CASE["bank_rows"], 512)
    dec = O.DeCapOracle(W.synth_decap(CASE["seed_dec"], prefix_size=512))
    orc = O.PatchionerOracle(tower(tag), dec, bank / bank.norm(dim=-1, keepdim=True), ClipDetokenizer().decode, normalize=False,
                             crop_dim=TOWERS[tag]["crop"])
    return orc, dec
