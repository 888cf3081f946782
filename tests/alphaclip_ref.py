"""Float reference of the AlphaCLIP backbone path (P/src/alphaclip/alpha_clip/model.py:351-380, alpha_mask_utils.py, the region driver
P/src/model.py:1060-1354), composed from ``oracle.patchioner_oracle``:

* the tower is ``ClipViTOracle`` (the OpenAI-CLIP ViT, arithmetic identical to AlphaCLIP's VisionTransformer) with a FOUR-channel
  patch convolution: conv1(x) + conv1_alpha(alpha) is one conv over [x; alpha] with the weights [conv1 | conv1_alpha] stacked on the
  input-channel axis;
* the masks are a host restatement of alpha_mask_utils.py (float32 box arithmetic with torch's own ``//``; traces through the
  oracle's map_traces_to_grid);
* the region driver loops one region per tower pass and caption call, as the reference does, over ``PatchionerOracle.caption_tokens``.

Also the shared inputs of tools/oracle/gen_golden_alphaclip.py and the AlphaCLIP tests (seeds, the box / trace table)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from oracle import patchioner_oracle as O

# ---- inputs shared by the fixture generator and the tests ---------------------------------------------------------------
CASE = dict(name="ViT-B/16", depth=2, seed_vit=71, seed_dec=73, seed_bank=75, seed_img=77, bank_rows=2048, B=2, crop=224, patch=16)

# xywh boxes in crop pixels: fractional, past the edges, zero-width / zero-height, negative origins, one-pixel, whole image
MASK_BOXES = [
    [0.0, 0.0, 224.0, 224.0], [10.5, 20.25, 30.75, 40.5], [15.9, 15.9, 0.2, 0.2], [15.99, 31.999, 16.02, 16.0],
    [200.0, 210.0, 50.0, 40.0], [-8.5, -3.0, 40.0, 20.0], [100.0, 100.0, 0.0, 30.0], [50.0, 60.0, 25.0, 0.0],
    [223.5, 223.5, 1.0, 1.0], [224.0, 10.0, 5.0, 5.0], [-30.0, 40.0, 20.0, 10.0], [31.0, 47.0, 1.0, 1.0],
    [0.3333333, 111.1, 99.99, 12.7], [160.0, 0.0, 64.0, 224.0],
]
MASK_TRACES = [
    [{"x": 0.0, "y": 0.0}, {"x": 1.0, "y": 1.0}, {"x": 0.5, "y": 0.5}],
    [{"x": -0.01, "y": 0.3}, {"x": 1.01, "y": 0.3}, {"x": 0.3, "y": 1.5}, {"x": 0.999999, "y": 0.0714285714}],
    [{"x": 0.1 + 0.013 * i, "y": 0.8 - 0.011 * i} for i in range(40)],
    [],
]


def region_boxes() -> torch.Tensor:
    """[B, 5, 4] boxes of the caption cases: real boxes of several sizes and one dummy (all -1) per image, in crop pixels."""
    return torch.tensor([[[10.0, 20.0, 60.0, 50.0], [-1.0, -1.0, -1.0, -1.0], [100.5, 30.25, 80.0, 120.75], [0.0, 0.0, 224.0, 224.0],
                          [150.0, 150.0, 100.0, 100.0]],
                         [[40.0, 40.0, 16.0, 16.0], [5.0, 180.0, 200.0, 30.0], [-1.0, -1.0, -1.0, -1.0], [64.0, 0.0, 32.0, 224.0],
                          [120.0, 60.0, 0.0, 40.0]]], dtype=torch.float32)


def region_traces() -> List[List[dict]]:
    return [[{"x": 0.2 + 0.02 * i, "y": 0.3 + 0.015 * i} for i in range(25)],
            [{"x": 0.7 - 0.01 * i, "y": 0.6 + 0.012 * (i % 7)} for i in range(30)]]


# ---- masks (alpha_mask_utils.py) -------------------------------------------------------------------------------------------
def box_mask(box: Sequence[float], grid: int, divisor: int) -> torch.Tensor:
    """bbox_to_alpha_mask: float32 ends, torch's float floor division, clamps, exclusive end."""
    b = torch.tensor([float(v) for v in box], dtype=torch.float32)
    x_min, y_min, w, h = b
    x1, y1 = int(x_min // divisor), int(y_min // divisor)
    x2, y2 = int((x_min + w) // divisor), int((y_min + h) // divisor)
    x1, y1 = max(0, min(x1, grid - 1)), max(0, min(y1, grid - 1))
    x2, y2 = max(0, min(x2, grid)), max(0, min(y2, grid))
    m = torch.zeros(grid, grid, dtype=torch.uint8)
    if x2 > x1 and y2 > y1:
        m[y1:y2, x1:x2] = 1
    return m


def trace_mask(points: Sequence[dict], grid: int) -> torch.Tensor:
    """trace_to_alpha_mask: map_traces_to_grid, made binary."""
    return (O.map_traces_to_grid(points, grid) > 0).to(torch.uint8)


def region_mask(boxes: Sequence[Sequence[float]], points: Sequence[dict], grid: int, divisor: int) -> torch.Tensor:
    m = torch.zeros(grid, grid, dtype=torch.uint8)
    for b in boxes:
        m |= box_mask(b, grid, divisor)
    if len(points):
        m |= trace_mask(points, grid)
    return m


# ---- the tower ---------------------------------------------------------------------------------------------------------------
class AlphaClipViTOracle(O.ClipViTOracle):
    """AlphaCLIP's VisionTransformer over engine-layout weights (weights.alphaclip_to_engine): ClipViTOracle with the alpha mask as a
    fourth input channel.  ``alpha`` [B, 1, S, S] float (None: ones, the whole-image forward)."""

    def __init__(self, engine_sd: Dict[str, torch.Tensor], num_heads: int = 12, patch_size: int = 16):
        w = dict(engine_sd)
        w["patch_embed.proj.weight"] = torch.cat([w["patch_embed.proj.weight"].float(), w.pop("patch_embed.alpha.weight").float()], dim=1)
        super().__init__(w, num_heads=num_heads, patch_size=patch_size)

    def __call__(self, imgs: torch.Tensor, alpha: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        if alpha is None:
            alpha = torch.ones(imgs.shape[0], 1, imgs.shape[2], imgs.shape[3])
        return super().__call__(torch.cat([imgs.float(), alpha.float()], dim=1))

    def tokens(self, imgs, alpha=None) -> torch.Tensor:
        d = self(imgs, alpha)
        return torch.cat([d["x_norm_clstoken"][:, None], d["x_norm_patchtokens"]], 1)


# ---- the region driver -------------------------------------------------------------------------------------------------------
class AlphaClipRef:
    """forward_alphaclip_with_regions over the oracle: one tower pass and one caption call per region, in the reference's order."""

    def __init__(self, vit: AlphaClipViTOracle, orc: "O.PatchionerOracle", crop: int = 224, use_cls: bool = True):
        self.vit, self.orc, self.crop, self.use_cls = vit, orc, crop, use_cls
        self.p = vit.patch_size
        self.tokens_log = None           # tests: a list collects the tower tokens of every region

    def feats(self, img, boxes, points):
        n = self.crop // self.p
        pix = region_mask(boxes, points, self.crop, 1).float()
        out = self.vit.tokens(img[None], pix[None, None])
        if self.tokens_log is not None:
            self.tokens_log.append(out[0].clone())
        if self.use_cls:
            return out[:, 0]
        cells = region_mask(boxes, points, n, self.p).float().view(1, -1)
        return (out[:, 1:] * cells.unsqueeze(-1)).sum(dim=1) / (cells.sum(dim=1, keepdim=True) + 1e-8)

    def forward(self, imgs, bboxes=None, traces=None, get_controllable_capts=False, compute_scores=False):
        outs = {}
        bs = imgs.shape[0]
        if get_controllable_capts:
            caps = []
            for i in range(bs):
                boxes = [b.tolist() for b in bboxes[i] if not float(b.sum()) < 0] if bboxes is not None else []
                pts = [p for tr in traces[i] for p in tr] if traces is not None else []
                ret = self.orc.caption_tokens(self.feats(imgs[i], boxes, pts), compute_scores=compute_scores)
                caps += ret[0] if compute_scores else ret
            return {"set_controllable_capts": caps}
        if bboxes is not None:
            outs["bbox_capts"], scores = [], []
            for i in range(bs):
                caps, sc = [], []
                for b in bboxes[i]:
                    if float(b.sum()) < 0:
                        caps.append("")
                        sc.append(0.0)
                        continue
                    ret = self.orc.caption_tokens(self.feats(imgs[i], [b.tolist()], []), compute_scores=compute_scores)
                    caps += ret[0] if compute_scores else ret
                    if compute_scores:
                        sc += ret[1]
                outs["bbox_capts"].append(caps)
                scores.append(sc)
            if compute_scores:
                outs["bbox_scores"] = scores
        if traces is not None:
            outs["trace_capts"], scores = [], []
            for i in range(bs):
                ret = self.orc.caption_tokens(self.feats(imgs[i], [], traces[i]), compute_scores=compute_scores)
                outs["trace_capts"] += ret[0] if compute_scores else ret
                if compute_scores:
                    scores += ret[1]
            if compute_scores:
                outs["trace_scores"] = scores
        return outs
