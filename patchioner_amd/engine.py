"""Thin python owner of one libpatchioner_hip handle: torch tensors in, torch tensors out.

PyTorch here only provides device memory (tensors), the current stream and (in ``dist.py``)
``torch.distributed``; every computation is a C-ABI call into the HIP library.  One Engine per process /
GPU; not re-entrant (same as the reference, whose hooks write module-level globals,
P/src/dino_extraction.py:7, P/src/model.py:30).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import PioConfig, PioError, check, ptr


# Steps per segment of a stop_at_eos decode: the segment length with the lowest mean forward() time over the captions-end-by-column-9 and
# -18 cases of tools/microbench/stop_at_eos_probe.py (1, 2 and 4 lie within 0.06 ms of each other; 8 is 0.5 ms behind).
DEFAULT_STOP_SEGMENT = 2


def _stop_ids(stop_ids, most: int):
    """None, or [id0, id1] (id1 = -1: one stop id) of 1..``most`` non-negative token ids."""
    if stop_ids is None:
        return None
    ids = [int(i) for i in stop_ids]
    if not 1 <= len(ids) <= most or min(ids) < 0:
        raise ValueError("stop ids: 1..%d non-negative token ids (%r)" % (most, stop_ids))
    return ids + [-1] * (2 - len(ids))


def _stop_seg(seg) -> int:
    seg = DEFAULT_STOP_SEGMENT if seg is None else int(seg)
    if seg < 1:
        raise ValueError("the segment of a stop_at_eos decode is >= 1 steps (%r)" % (seg,))
    return seg


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class Engine:
    # The sparse last block is taken while the selected rows stay below 1 / SPARSE_SHARE_DEN of the launch's padded rows: the library's
    # kSparseShareDen (kernels.h), which also sizes its workspace.  One half until the cut-over is measured.
    SPARSE_SHARE_DEN = 2

    def __init__(self, *, embed_dim: int, depth: int, num_heads: int, num_registers: int, crop_dim: int,
                 patch_size: int = 14, pretrain_grid: int = 37, prefix_size: int = 768, dec_layers: int = 4,
                 dec_heads: int = 4, dec_embd: int = 768, dec_vocab: int = 50257, dec_positions: int = 1024,
                 max_batch: int = 16, max_prefixes: int = 64, max_steps: int = 30, vit_dtype: str = "fp16",
                 device_index: int = 0, readout_heads: int = 16, readout_scale: float = 0.125, vit_arch: str = "dinov2",
                 vit_out_dim: int = 0, vit_ln_eps: float = 1e-6, rn_layers=(0, 0, 0, 0), rn_width: int = 0,
                 rn_attnpool_spatial: bool = True, vit_self_only_layers: int = 0, sparse_clip_tail: bool = False):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise PioError(-101, "no HIP device visible: the captioning path has no CPU fallback")
        self.device = torch.device("cuda", device_index)
        cfg = PioConfig(
            embed_dim=embed_dim, depth=depth, num_heads=num_heads, patch_size=patch_size,
            num_registers=num_registers, pretrain_grid=pretrain_grid, crop_dim=crop_dim, vit_ln_eps=vit_ln_eps,
            readout_heads=readout_heads, readout_scale=readout_scale, dec_layers=dec_layers, dec_heads=dec_heads,
            dec_embd=dec_embd, dec_vocab=dec_vocab, dec_positions=dec_positions, prefix_size=prefix_size,
            dec_ln_eps=1e-5, max_batch=max_batch, max_prefixes=max_prefixes, max_steps=max_steps,
            vit_operand_type={"fp16": 0, "bf16": 1, "fp32": 2}[vit_dtype], device=device_index,
            vit_arch={"dinov2": 0, "clip": 1, "alphaclip": 2, "regionclip": 3}[vit_arch], vit_out_dim=vit_out_dim,
            rn_layers=(ctypes.c_int32 * 4)(*rn_layers), rn_width=rn_width, rn_attnpool_spatial=int(bool(rn_attnpool_spatial)),
            vit_self_only_layers=int(vit_self_only_layers))
        self.cfg = cfg
        h = ctypes.c_void_p()
        check(self.lib.pio_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        # D = width of the tokens the backbone returns (the CLIP ViT's head maps embed_dim -> vit_out_dim); Dv = its own width
        self.D, self.G, self.Dv = (vit_out_dim or embed_dim), 1 + num_registers, embed_dim
        self.vit_arch = vit_arch
        self.n = self.lib.pio_grid_side(h)
        self.T = self.lib.pio_num_tokens(h)
        self.n2 = self.n * self.n
        self.prefix_size = prefix_size
        self.max_batch, self.max_prefixes, self.max_steps = max_batch, max_prefixes, max_steps
        self.num_weights = 0
        self.last_steps_run = None      # steps every chunk of the last stop_at_eos decode ran (decode_greedy / viecap_decode with stop ids)
        self.bank_rows = 0
        self.bank_dim = 0
        self._finalized = False
        self._stage_ring = [dict(host=None, dev=None, event=None) for _ in range(8)]
        self.Tp = (self.T + 7) // 8 * 8          # padded rows per image of the token matrix
        # the sparse last block (pio_vit_forward_rows): fp16 / bf16 DINOv2 towers; the plain CLIP ViT (no self-only block), whose tail is
        # the last block, ln_post and the head, only when the caller asks for it (sparse_clip_tail)
        self.sparse_ok = (vit_dtype in ("fp16", "bf16") and not vit_self_only_layers
                          and (vit_arch == "dinov2" or (vit_arch == "clip" and bool(sparse_clip_tail))))
        self._stage_next = 0

    def close(self):
        """Destroys the handle.  An engine that still has live decoder clones is refused by the library (the clones borrow
        its weights): the handle is kept and the error raised, so that nothing leaks silently."""
        if getattr(self, "h", None) is not None and self.h.value:
            check(self.lib.pio_destroy(self.h))
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clone_decoder(self) -> "DecoderClone":
        """A second greedy decoder on this engine's weights (pio_clone_decoder): own KV caches / scratch / graphs, so its
        decode_greedy may run concurrently with this engine's on another stream.  Close it before this engine."""
        return DecoderClone(self)

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False) -> List[str]:
        """Upload fp32 tensors under their checkpoint keys; returns the keys the library does not know."""
        unknown = []
        for k, v in sd.items():
            t = v.detach().to(dtype=torch.float32, device="cpu").contiguous()
            shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
            rc = self.lib.pio_load_weight(self.h, k.encode(), ptr(t), shape, t.dim())
            if rc == _lib.PIO_ERR_UNKNOWN_WEIGHT:
                unknown.append(k)
                continue
            check(rc)
            self.num_weights += t.numel()
        if strict and unknown:
            raise PioError(_lib.PIO_ERR_UNKNOWN_WEIGHT, "unexpected keys: %s" % unknown[:8])
        return unknown

    def finalize(self):
        check(self.lib.pio_finalize_weights(self.h))
        self._finalized = True

    def set_memory_bank(self, bank: torch.Tensor) -> int:
        bank = bank.detach().to(torch.float32).contiguous()
        if bank.is_cuda:
            # the reference drops zero-norm rows when it loads the bank (im2txtprojection.py:343-345); a zero row would
            # give inv_norm = inf and NaN similarities
            keep = bank.norm(dim=-1) != 0
            if not bool(keep.all()):
                bank = bank[keep].contiguous()
            check(self.lib.pio_set_memory_bank_device(self.h, ptr(bank), bank.shape[0], bank.shape[1]))
        else:
            kept = ctypes.c_int64(0)
            check(self.lib.pio_set_memory_bank(self.h, ptr(bank), bank.shape[0], bank.shape[1], ctypes.byref(kept)))
        self.bank_rows = int(self.lib.pio_bank_rows(self.h))
        self.bank_dim = int(bank.shape[1])
        return self.bank_rows

    def bank_form(self) -> str:
        """"split" (fp16 hi + lo operands) or "exact" (fp32): the form project() takes on the loaded bank (pio_bank_form)."""
        f = int(self.lib.pio_bank_form(self.h))
        if f < 0:
            raise PioError(-3, "memory bank not set")
        return "split" if f else "exact"

    # ------------------------------------------------------------------ measurement
    PROFILE_CLASSES = {"vit_gemm": 0, "vit_attention": 1, "vit_layernorm": 2, "mem_project": 3, "decode": 4}

    def profile_enable(self, on: bool = True):
        check(self.lib.pio_profile_enable(self.h, 1 if on else 0))

    def profile_read(self) -> Dict[str, dict]:
        out = {}
        for name, cls in self.PROFILE_CLASSES.items():
            ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            check(self.lib.pio_profile_read(self.h, cls, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl),
                                            ctypes.byref(by)))
            out[name] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
        return out

    # ------------------------------------------------------------------ a2/a3 backbone
    def _dev(self, t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        return t.to(device=self.device, dtype=dtype).contiguous()

    def vit_forward(self, imgs: torch.Tensor, want_qkv: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        imgs = self._dev(imgs)
        B = imgs.shape[0]
        crop = self.cfg.crop_dim
        if tuple(imgs.shape[1:]) != (3, crop, crop):
            # the reference's reshape in process_self_attention fails for any other size
            raise ValueError("images must be [B,3,%d,%d], got %s" % (crop, crop, tuple(imgs.shape)))
        tokens = torch.empty(B, self.T, self.D, device=self.device, dtype=torch.float32)
        if want_qkv and self.vit_arch != "dinov2":
            raise PioError(_lib.PIO_ERR_INVALID_ARG, "the CLIP ViT exposes no qkv hook (P/src/model.py:864-865)")
        qkv = torch.empty(B, self.T, 3 * self.Dv, device=self.device, dtype=torch.float32) if want_qkv else None
        for s in range(0, B, self.max_batch):
            e = min(B, s + self.max_batch)
            check(self.lib.pio_vit_forward(self.h, ptr(imgs[s:e]), e - s, ptr(tokens[s:e]),
                                           ptr(qkv[s:e]) if want_qkv else None, _stream()))
        return tokens, qkv

    def region_masks(self, regions: Sequence[Tuple[Sequence[Sequence[float]], Sequence[Tuple[float, float]]]], grid: int,
                     divisor: int) -> torch.Tensor:
        """AlphaCLIP region masks on the device (pio_region_masks): ``regions`` = one (boxes [[x, y, w, h], ...], points [(x, y), ...])
        pair per region, the mask being their union -> uint8 [R, grid, grid] (0 / 1).  One table upload, one launch."""
        R = len(regions)
        boxes = np.array([b for bx, _ in regions for b in bx], dtype=np.float32).reshape(-1, 4)
        pts = np.array([q for _, pt in regions for q in pt], dtype=np.float64).reshape(-1, 2)
        if not np.isfinite(boxes).all():        # int() of a NaN / inf box end fails in bbox_to_alpha_mask; such trace points are skipped
            raise ValueError("cannot convert float NaN / inf box coordinates to integer")
        box_off = np.zeros(R + 1, dtype=np.int32)
        pt_off = np.zeros(R + 1, dtype=np.int32)
        np.cumsum([len(bx) for bx, _ in regions], out=box_off[1:])
        np.cumsum([len(pt) for _, pt in regions], out=pt_off[1:])
        bd = torch.from_numpy(boxes).to(self.device) if len(boxes) else None
        pd = torch.from_numpy(pts).to(self.device) if len(pts) else None
        bo, po = torch.from_numpy(box_off).to(self.device), torch.from_numpy(pt_off).to(self.device)
        out = torch.empty(R, grid, grid, device=self.device, dtype=torch.uint8)
        check(self.lib.pio_region_masks(self.h, ptr(bd), ptr(bo), ptr(pd), ptr(po), R, int(grid), float(divisor), ptr(out), _stream()))
        return out

    def vit_forward_regions(self, imgs: torch.Tensor, img_of_region: torch.Tensor, masks: Optional[torch.Tensor]) -> torch.Tensor:
        """AlphaCLIP: one tower pass per region (pio_vit_forward_regions), region r on image img_of_region[r] with the alpha mask
        masks[r] (uint8 [R, S, S]; None: ones) -> tokens [R, T, D], in launches of at most max_batch regions."""
        imgs = self._dev(imgs)
        crop = self.cfg.crop_dim
        if tuple(imgs.shape[1:]) != (3, crop, crop):
            raise ValueError("images must be [B,3,%d,%d], got %s" % (crop, crop, tuple(imgs.shape)))
        idx = self._dev(img_of_region, torch.int32)
        R = int(idx.shape[0])
        if R and (int(idx.min()) < 0 or int(idx.max()) >= imgs.shape[0]):
            raise IndexError("img_of_region outside the %d images of the call" % imgs.shape[0])
        if masks is not None:
            masks = masks.to(device=self.device, dtype=torch.uint8).contiguous()
            if tuple(masks.shape) != (R, crop, crop):
                raise ValueError("masks must be [R,%d,%d], got %s" % (crop, crop, tuple(masks.shape)))
        tokens = torch.empty(R, self.T, self.D, device=self.device, dtype=torch.float32)
        for s in range(0, R, self.max_batch):
            e = min(R, s + self.max_batch)
            check(self.lib.pio_vit_forward_regions(self.h, ptr(imgs), ptr(idx[s:e]), ptr(masks[s:e]) if masks is not None else None,
                                                   e - s, ptr(tokens[s:e]), _stream()))
        return tokens

    # ------------------------------------------------------------------ a4/a5 read-out
    def cls_attention(self, qkv: torch.Tensor, tokens: torch.Tensor, want_maps=False, want_avg=False,
                      want_disentangled=False):
        B = qkv.shape[0]
        Hr = self.cfg.readout_heads
        self_attn = torch.empty(B, self.n2, device=self.device, dtype=torch.float32)
        maps = torch.empty(B, Hr, self.n2, device=self.device, dtype=torch.float32) if want_maps else None
        avg = torch.empty(B, self.D, device=self.device, dtype=torch.float32) if want_avg else None
        dis = torch.empty(B, Hr, self.D, device=self.device, dtype=torch.float32) if want_disentangled else None
        for s in range(0, B, self.max_batch):
            e = min(B, s + self.max_batch)
            sl = slice(s, e)
            check(self.lib.pio_cls_attention(
                self.h, ptr(qkv[sl]), ptr(tokens[sl]), e - s, ptr(self_attn[sl]),
                ptr(maps[sl]) if want_maps else None, ptr(avg[sl]) if want_avg else None,
                ptr(dis[sl]) if want_disentangled else None, _stream()))
        return self_attn, maps, avg, dis

    # ------------------------------------------------------------------ a6 traces
    def trace_grids(self, traces: Sequence[Sequence[dict]], select_rows: bool = False):
        """map_traces_to_grid for a batch: points packed CSR-style into ONE pinned staging buffer (x, y as
        float64 followed by the int32 offsets) and sent with one asynchronous copy; the counting runs on
        the device.  A ring of 8 staging slots (each guarded by an event) lets the host run several batches
        ahead of the GPU without overwriting a buffer whose copy has not executed yet.

        ``select_rows``: returns (grids, sel).  The rows of the token matrix whose patches received a point are selected on the
        host from the staged points (pio_host_trace_quads, the device's cell arithmetic) and kept in the same staging slot; ``sel``
        is what vit_forward_rows takes, or None when the sparse last block does not apply (nothing selected, more than
        1 / SPARSE_SHARE_DEN of the rows, more images than one launch holds)."""
        B = len(traces)
        xy = np.array([(p["x"], p["y"]) for tr in traces for p in tr], dtype=np.float64).reshape(-1, 2)
        npts = xy.shape[0]
        nbytes = npts * 16 + (B + 1) * 4
        qcap = B * self.Tp // 4 if select_rows else 0
        sel_bytes = (B + 1 + qcap) * 4           # img_off [B + 1] | quads [<= B Tp / 4], behind the uploaded part
        slot = self._stage_ring[self._stage_next % len(self._stage_ring)]
        self._stage_next += 1
        if slot["event"] is not None:
            slot["event"].synchronize()
        if slot["host"] is None or slot["host"].numel() < nbytes + sel_bytes:
            cap = max(1 << 16, 2 * (nbytes + sel_bytes))
            slot["host"] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            slot["dev"] = torch.empty(cap, dtype=torch.uint8, device=self.device)
        host = slot["host"].numpy()
        host[: npts * 16].view(np.float64)[:] = xy.reshape(-1)
        offs = host[npts * 16: nbytes].view(np.int32)
        offs[0] = 0
        np.cumsum([len(tr) for tr in traces], out=offs[1:])
        slot["dev"][:nbytes].copy_(slot["host"][:nbytes], non_blocking=True)
        base = slot["dev"].data_ptr()
        grids = torch.empty(B, self.n, self.n, device=self.device, dtype=torch.float32)
        check(self.lib.pio_trace_grids(self.h, base if npts else None, base + npts * 16, B, npts, ptr(grids), _stream()))
        if slot["event"] is None:
            slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream())
        if not select_rows:
            return grids
        sel = None
        if self.sparse_ok and B <= self.max_batch:
            hbase = slot["host"].data_ptr()
            nq = self.lib.pio_host_trace_quads(hbase if npts else None, hbase + npts * 16, B, self.n, self.G, self.Tp,
                                               hbase + nbytes + (B + 1) * 4, qcap, hbase + nbytes)
            if nq < 0:
                check(nq)
            if 0 < nq and 4 * nq * self.SPARSE_SHARE_DEN < B * self.Tp:
                sel = dict(slot=slot, img_off=hbase + nbytes, quads=hbase + nbytes + (B + 1) * 4, nq=int(nq), B=B)
        return grids, sel

    def vit_forward_rows(self, imgs: torch.Tensor, sel: dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """The backbone with the sparse last block (pio_vit_forward_rows) for the rows ``sel`` lists (trace_grids(select_rows=True)
        of the same images, in order) -> (compact final tokens [4 nq, D], row_map int32 [B, n2] for region_reduce_rows)."""
        imgs = self._dev(imgs)
        B, crop = imgs.shape[0], self.cfg.crop_dim
        if tuple(imgs.shape[1:]) != (3, crop, crop) or B != sel["B"]:
            raise ValueError("images must be [%d,3,%d,%d], got %s" % (sel["B"], crop, crop, tuple(imgs.shape)))
        tokens = torch.empty(4 * sel["nq"], self.D, device=self.device, dtype=torch.float32)
        row_map = torch.empty(B, self.n2, device=self.device, dtype=torch.int32)
        check(self.lib.pio_vit_forward_rows(self.h, ptr(imgs), B, sel["quads"], sel["img_off"], ptr(tokens), ptr(row_map), _stream()))
        sel["slot"]["event"].record(torch.cuda.current_stream())      # the list is copied from the staging slot on this stream
        return tokens, row_map

    def region_reduce_rows(self, tokens: torch.Tensor, row_map: torch.Tensor, weights: torch.Tensor, scale: float) -> torch.Tensor:
        """region_reduce over the compact tokens of vit_forward_rows: row r of ``weights`` weighs the patches of the image whose map
        is row r of ``row_map`` (a slice of the launch's map)."""
        weights = self._dev(weights.reshape(-1, self.n2))
        R = weights.shape[0]
        assert row_map.shape[0] == R and row_map.is_contiguous()
        out = torch.empty(R, self.D, device=self.device, dtype=torch.float32)
        check(self.lib.pio_region_reduce_rows(self.h, ptr(tokens), ptr(row_map), ptr(weights), None, R, float(scale), ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ a7 boxes
    def bbox_weights(self, boxes_i32: torch.Tensor, mode: int, variance: float = 0.5,
                     center_choice: Optional[torch.Tensor] = None, attn: Optional[torch.Tensor] = None,
                     single_map: bool = False):
        """boxes_i32 [B,NB,4] int32 (already // patch_size); returns (weights [B,NB,n2], single [B,n2] | None)."""
        boxes_i32 = self._dev(boxes_i32, torch.int32)
        B, NB = boxes_i32.shape[:2]
        weights = torch.empty(B, NB, self.n2, device=self.device, dtype=torch.float32)
        single = torch.empty(B, self.n2, device=self.device, dtype=torch.float32) if single_map else None
        cc = self._dev(center_choice, torch.int32) if center_choice is not None else None
        check(self.lib.pio_bbox_weights(self.h, ptr(boxes_i32), B, NB, mode, float(variance), ptr(cc), ptr(attn),
                                        ptr(weights), 1 if single_map else 0, ptr(single), _stream()))
        return weights, single

    def preprocess(self, images: Sequence, resize_dim: int, crop_dim: int, no_crop: bool = False) -> torch.Tensor:
        """image_transforms / image_transforms_no_crop (P/src/model.py:347-357) for a list of RGB images of different
        sizes (PIL images or uint8 [H][W][3] arrays / tensors) -> fp32 [B][3][S][S] on the device, bit-exact to the
        host PIL pipeline.  The raw pixels cross PCIe once (pinned staging, one asynchronous copy); resize, crop and
        normalisation run on the GPU (pio_preprocess)."""
        arrs = []
        for im in images:
            if isinstance(im, torch.Tensor):
                a = im.detach().cpu().numpy()
            elif isinstance(im, np.ndarray):
                a = im
            else:
                a = np.asarray(im.convert("RGB"))
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("preprocess expects RGB uint8 [H][W][3] images")
            arrs.append(np.ascontiguousarray(a))
        B = len(arrs)
        sizes = np.array([(a.shape[1], a.shape[0]) for a in arrs], dtype=np.int32)
        nbytes = [a.size for a in arrs]
        offsets = np.zeros(B, dtype=np.int64)
        offsets[1:] = np.cumsum([(n + 15) // 16 * 16 for n in nbytes])[:-1]
        total = int(offsets[-1] + nbytes[-1])
        slot = self._stage_ring[self._stage_next % len(self._stage_ring)]
        self._stage_next += 1
        if slot["event"] is not None:
            slot["event"].synchronize()
        if slot["host"] is None or slot["host"].numel() < total:
            cap = max(1 << 16, 2 * total)
            slot["host"] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            slot["dev"] = torch.empty(cap, dtype=torch.uint8, device=self.device)
        host = slot["host"].numpy()
        for a, o, n in zip(arrs, offsets, nbytes):
            host[o:o + n] = a.reshape(-1)
        slot["dev"][:total].copy_(slot["host"][:total], non_blocking=True)
        S = resize_dim if no_crop else crop_dim
        out = torch.empty(B, 3, S, S, device=self.device, dtype=torch.float32)
        check(self.lib.pio_preprocess(self.h, slot["dev"].data_ptr(), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                      sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), B, int(resize_dim), int(crop_dim),
                                      1 if no_crop else 0, ptr(out), _stream()))
        if slot["event"] is None:
            slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream())
        return out

    def region_reduce(self, tokens: torch.Tensor, weights: torch.Tensor, img_index: Optional[torch.Tensor],
                      scale: float) -> torch.Tensor:
        """out[r] = scale * sum_p weights[r,p] * patch_tokens[img_index[r], p]"""
        weights = self._dev(weights.reshape(-1, self.n2))
        R = weights.shape[0]
        idx = self._dev(img_index, torch.int32) if img_index is not None else None
        out = torch.empty(R, self.D, device=self.device, dtype=torch.float32)
        check(self.lib.pio_region_reduce(self.h, ptr(tokens), tokens.shape[0], ptr(weights), ptr(idx), R, float(scale),
                                         ptr(out), _stream()))
        return out

    def bbox_double_dino(self, tokens: torch.Tensor, slices: torch.Tensor, use_cls: bool, return_type: str) -> torch.Tensor:
        """extract_bboxes_feats_double_dino, return types "cls" / "avg" (P/src/bbox_utils.py:300-403): the last ViT block
        re-run on [cls | registers | region patches] of every box.  ``slices`` int32 [B, NB, 4] = python-normalised
        (y_start, y_end, x_start, x_end) patch-grid slices.  -> [B, NB, D]."""
        B, NB = slices.shape[:2]
        sl = self._dev(slices.reshape(-1, 4), torch.int32)
        out = torch.empty(B * NB, self.D, device=self.device, dtype=torch.float32)
        check(self.lib.pio_bbox_double_dino(self.h, ptr(tokens), ptr(sl), B, NB, 1 if use_cls else 0,
                                            {"cls": 0, "avg": 1}[return_type], ptr(out), _stream()))
        return out.view(B, NB, self.D)

    def ctx_clean(self, dirty: torch.Tensor, ctx: torch.Tensor, cleaning_type: str, alpha: float,
                  normalize_inputs: bool = False) -> torch.Tensor:
        """Patchioner.ctx_cleaner (P/src/model.py:1425-1436): dirty [B, S, D], ctx [B, D] -> cleaned [B, S, D];
        ``normalize_inputs`` L2-normalises both first (model.py:907-913)."""
        dirty, ctx = self._dev(dirty), self._dev(ctx)
        B, S, D = dirty.shape
        out = torch.empty_like(dirty)
        check(self.lib.pio_ctx_clean(self.h, ptr(dirty), ptr(ctx), B * S, D, S,
                                     {"orthogonal_projection": 0, "contrastive_mask": 1}[cleaning_type], float(alpha),
                                     1 if normalize_inputs else 0, ptr(out), _stream()))
        return out

    def project_many(self, q: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """project() for any number of queries [N, D] (in-place L2 normalisation of q, like project): chunks of
        max_prefixes rows, one pass over the bank per 16 of them."""
        assert q.is_cuda and q.dtype == torch.float32 and q.is_contiguous()
        out = torch.empty_like(q)
        for s in range(0, q.shape[0], self.max_prefixes):
            out[s:s + self.max_prefixes] = self.project(q[s:s + self.max_prefixes], normalize=normalize)
        return out

    def gaussian_map(self, variance: float) -> torch.Tensor:
        m = torch.empty(self.n2, device=self.device, dtype=torch.float32)
        check(self.lib.pio_gaussian_map(self.h, float(variance), ptr(m), _stream()))
        return m

    # ------------------------------------------------------------------ a9/a10 projection
    def project(self, q: torch.Tensor, temperature: float = 0.01, normalize: bool = False,
                n_best: Optional[int] = None):
        """q [N,D] CUDA fp32 contiguous is L2-normalised IN PLACE (reference quirk)."""
        assert q.is_cuda and q.dtype == torch.float32 and q.is_contiguous()
        if q.shape[1] != self.bank_dim:        # the kernel strides q / out by the bank's width
            raise PioError(_lib.PIO_ERR_SHAPE, "query width %d does not match the %d-wide memory bank" % (q.shape[1], self.bank_dim))
        N = q.shape[0]
        out = torch.empty(N, q.shape[1], device=self.device, dtype=torch.float32)
        nb = int(n_best) if n_best else 0
        best = torch.empty(N, nb, device=self.device, dtype=torch.float32) if nb else None
        check(self.lib.pio_mem_project(self.h, ptr(q), N, float(temperature), 1 if normalize else 0, ptr(out), nb,
                                       ptr(best), _stream()))
        return (out, best) if nb else out

    def topk_rows(self, q: torch.Tensor, k: int = 1):
        """project(..., return_argmax_text=True, return_n_best_sims=k) without the texts: q [N, D] is L2-normalised IN PLACE,
        returns (sims [N, k] descending, rows [N, k] int64) of the k most similar bank rows per query."""
        assert q.is_cuda and q.dtype == torch.float32 and q.is_contiguous()
        if q.shape[1] != self.bank_dim:
            raise PioError(_lib.PIO_ERR_SHAPE, "query width %d does not match the %d-wide memory bank" % (q.shape[1], self.bank_dim))
        N = q.shape[0]
        sims = torch.empty(N, k, device=self.device, dtype=torch.float32)
        rows = torch.empty(N, k, device=self.device, dtype=torch.int64)
        for s in range(0, N, self.max_prefixes):
            e = min(N, s + self.max_prefixes)
            check(self.lib.pio_mem_topk(self.h, ptr(q[s:e]), e - s, int(k), ptr(sims[s:e]), ptr(rows[s:e]), _stream()))
        return sims, rows

    ACTS = {None: 0, "none": 0, "relu": 1, "tanh": 2, "sigmoid": 3}

    def text_project(self, x: torch.Tensor, w1, b1, w2=None, b2=None, act="tanh") -> torch.Tensor:
        """ProjectionLayer.project_clip_txt (P/src/talk2dino/talk2dino.py:73-83): x [N, in] CLIP text features ->
        hidden_layer(act(linear_layer(x))) [N, out] (linear_layer alone without w2), exact fp32 on the device."""
        x, w1, b1 = self._dev(x), self._dev(w1), self._dev(b1)
        N, out_dim = x.shape[0], w1.shape[0]
        if w1.shape[1] != x.shape[1] or b1.shape != (out_dim,):
            raise PioError(_lib.PIO_ERR_SHAPE, "linear_layer %s does not take %d-wide features" % (tuple(w1.shape), x.shape[1]))
        out = torch.empty(N, out_dim, device=self.device, dtype=torch.float32)
        hid = None
        if w2 is not None:
            w2, b2 = self._dev(w2), self._dev(b2)
            if w2.shape != (out_dim, out_dim) or b2.shape != (out_dim,):
                raise PioError(_lib.PIO_ERR_SHAPE, "hidden layer %s is not [%d, %d]" % (tuple(w2.shape), out_dim, out_dim))
            hid = torch.empty_like(out)
        check(self.lib.pio_text_project(self.h, ptr(x), N, x.shape[1], ptr(w1), ptr(b1), out_dim, ptr(w2) if w2 is not None else None,
                                        ptr(b2) if w2 is not None else None, self.ACTS[act], ptr(hid) if hid is not None else None,
                                        ptr(out), _stream()))
        return out

    def revert_transformation(self, x: torch.Tensor) -> torch.Tensor:
        x = self._dev(x)
        out = torch.empty(x.shape[0], self.prefix_size, device=self.device, dtype=torch.float32)
        check(self.lib.pio_revert_transformation(self.h, ptr(x), x.shape[0], ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ f1 ViECap head
    def viecap_set_entities(self, emb: torch.Tensor) -> None:
        t = emb.detach().to(dtype=torch.float32, device="cpu").contiguous()
        check(self.lib.pio_viecap_set_entities(self.h, ptr(t), t.shape[0], t.shape[1]))
        self.viecap_entities = int(t.shape[0])

    def viecap_mapping(self, feats: torch.Tensor) -> torch.Tensor:
        """feats [N, C] CUDA fp32 contiguous, L2-normalised IN PLACE -> soft prompt [N, Lc, E]."""
        assert feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous()
        N = feats.shape[0]
        Lc = self.lib.pio_viecap_prompt_length(self.h)
        out = torch.empty(N, Lc, self.cfg.dec_embd, device=self.device, dtype=torch.float32)
        for s in range(0, N, self.max_prefixes):
            e = min(N, s + self.max_prefixes)
            check(self.lib.pio_viecap_mapping(self.h, ptr(feats[s:e]), e - s, ptr(out[s:e]), _stream()))
        return out

    def viecap_entity_logits(self, feats: torch.Tensor, temperature: float) -> torch.Tensor:
        N = feats.shape[0]
        out = torch.empty(N, self.viecap_entities, device=self.device, dtype=torch.float32)
        check(self.lib.pio_viecap_entity_logits(self.h, ptr(feats), N, float(temperature), ptr(out), _stream()))
        return out

    def lm_score(self, rows) -> torch.Tensor:
        """Teacher-forced negative log-likelihood sums of token rows (list of lists of ids) under the language model
        (pio_lm_score): [N] float32 on the device; the reference's loss is this / (len - 1)."""
        N = len(rows)
        out = torch.empty(N, device=self.device, dtype=torch.float32)
        cap = min(self.max_prefixes, 64)
        for s in range(0, N, cap):
            chunk = rows[s:s + cap]
            L = max(1, max(len(r) for r in chunk))
            tok = torch.zeros(len(chunk), L, dtype=torch.int32)
            for i, r in enumerate(chunk):
                tok[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
            lens = torch.tensor([len(r) for r in chunk], dtype=torch.int32)
            tok_d, lens_d = self._dev(tok, torch.int32), self._dev(lens, torch.int32)
            check(self.lib.pio_lm_score(self.h, ptr(tok_d), ptr(lens_d), len(chunk), L, ptr(out[s:s + cap]), _stream()))
        return out

    def viecap_decode(self, cont: Optional[torch.Tensor], tokens: Optional[torch.Tensor], soft_first: bool = True, steps: int = 64,
                      stop_ids: Optional[Sequence[int]] = None, seg: Optional[int] = None) -> torch.Tensor:
        """cont [N, Lc, E] device (None: only_hard_prompt, the prompt is the tokens' word embeddings alone), tokens [N, Lt] int32
        (host or device) or None -> greedy ids [N, steps] int32.

        ``stop_ids`` (one or two ids; stop_at_eos): every chunk of max_prefixes rows runs in segments of ``seg`` steps (default
        DEFAULT_STOP_SEGMENT) and ends once each of its rows has emitted a stop id (pio_viecap_decode_stop: BLOCKING).  The ids are then
        the canonical table -- a row's first stop id repeated to the end of the row -- and ``last_steps_run`` lists the steps every
        chunk ran."""
        tok = self._dev(tokens, torch.int32) if tokens is not None else None
        if cont is None and tok is None:
            raise ValueError("viecap_decode: neither a soft prompt nor prompt tokens")
        stops = _stop_ids(stop_ids, 2)
        N = cont.shape[0] if cont is not None else tok.shape[0]
        Lt = int(tok.shape[1]) if tok is not None else 0
        ids = torch.empty(N, steps, device=self.device, dtype=torch.int32)
        ran = []
        for s in range(0, N, self.max_prefixes):
            e = min(N, s + self.max_prefixes)
            c = ptr(cont[s:e].contiguous()) if cont is not None else None
            t = ptr(tok[s:e].contiguous()) if tok is not None else None
            if stops is None:
                check(self.lib.pio_viecap_decode(self.h, c, t, e - s, Lt, 1 if soft_first else 0, int(steps), ptr(ids[s:e]), _stream()))
                continue
            n = ctypes.c_int32(0)
            check(self.lib.pio_viecap_decode_stop(self.h, c, t, e - s, Lt, 1 if soft_first else 0, int(steps), stops[0], stops[1],
                                                  _stop_seg(seg), ptr(ids[s:e]), ctypes.byref(n), _stream()))
            ran.append(int(n.value))
        if stops is not None:
            self.last_steps_run = ran
        return ids

    def viecap_compose_prompts(self, probs: torch.Tensor, frag, top_k: int, threshold: float, pad_id: int,
                               seg: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The hard prompt on the device (pio_viecap_compose_prompts): probs [N, K] (viecap_entity_logits), ``frag`` a
        viecap.PromptFragments on this device, ``seg`` [N] int32 caption call of every row (None: one call) -> token rows
        [N, frag.Lmax] int32 padded with ``pad_id`` and the per-row hard-prompt length [N] int32 (the call's longest row)."""
        assert probs.is_cuda and probs.dtype == torch.float32 and probs.is_contiguous()
        N, K = int(probs.shape[0]), int(probs.shape[1])
        if 2 * K != int(frag.off.numel()):
            raise ValueError("viecap_compose_prompts: %d entity probabilities per row, the fragment table has %d entities" % (K, frag.off.numel() // 2))
        if not 1 <= int(top_k) <= frag.top_k:
            raise ValueError("viecap_compose_prompts: top_k %d outside 1..%d, the table's bound (its Lmax holds %d entities)" % (top_k, frag.top_k, frag.top_k))
        tokens = torch.empty(N, frag.Lmax, device=self.device, dtype=torch.int32)
        lens = torch.empty(N, device=self.device, dtype=torch.int32)
        scratch = torch.empty(N, device=self.device, dtype=torch.int32)
        check(self.lib.pio_viecap_compose_prompts(self.h, ptr(probs), N, K, ptr(frag.ids), ptr(frag.off), ptr(frag.length), frag.head_off,
                                                  frag.head_len, frag.empty_off, frag.empty_len, int(top_k), float(threshold), int(pad_id),
                                                  ptr(seg) if seg is not None else None, frag.Lmax, ptr(tokens), ptr(lens), ptr(scratch),
                                                  _stream()))
        return tokens, lens

    def viecap_decode_ragged(self, cont: Optional[torch.Tensor], tokens: Optional[torch.Tensor], lens: Optional[torch.Tensor],
                             soft_first: bool = True, steps: int = 64) -> torch.Tensor:
        """viecap_decode with a hard-prompt length per row (pio_viecap_decode_ragged): cont [N, Lc, E] device or None (only_hard_prompt),
        tokens [N, Ltmax] int32 device, lens [N] int32 device (row n uses tokens[n, :lens[n]]), both None without a hard prompt ->
        greedy ids [N, steps] int32; row n's ids are those of viecap_decode on that row alone with its own lens[n] tokens."""
        if cont is None and tokens is None:
            raise ValueError("viecap_decode_ragged: neither a soft prompt nor prompt tokens")
        if (tokens is None) != (lens is None):
            raise ValueError("viecap_decode_ragged: tokens and lens go together")
        N = int(cont.shape[0] if cont is not None else tokens.shape[0])
        Lt = int(tokens.shape[1]) if tokens is not None else 0
        ids = torch.empty(N, steps, device=self.device, dtype=torch.int32)
        cap = min(self.max_prefixes, 128)                 # rows of one ragged decode
        for s in range(0, N, cap):
            e = min(N, s + cap)
            check(self.lib.pio_viecap_decode_ragged(self.h, ptr(cont[s:e].contiguous()) if cont is not None else None,
                                                    ptr(tokens[s:e].contiguous()) if tokens is not None else None,
                                                    ptr(lens[s:e].contiguous()) if lens is not None else None,
                                                    e - s, Lt, 1 if soft_first else 0, int(steps), ptr(ids[s:e]), _stream()))
        return ids

    def viecap_build_prompt(self, cont: Optional[torch.Tensor], tokens: Optional[torch.Tensor], soft_first: bool = True) -> torch.Tensor:
        """The prompt embeddings [N, Lc + Lt, E] as viecap_decode assembles them (word_embed + torch.cat, entrypoint.py:126-135)."""
        tok = self._dev(tokens, torch.int32) if tokens is not None else None
        if cont is None and tok is None:
            raise ValueError("viecap_build_prompt: neither a soft prompt nor prompt tokens")
        N = cont.shape[0] if cont is not None else tok.shape[0]
        Lt = int(tok.shape[1]) if tok is not None else 0
        Lc = int(cont.shape[1]) if cont is not None else 0
        out = torch.empty(N, Lc + Lt, self.cfg.dec_embd, device=self.device, dtype=torch.float32)
        check(self.lib.pio_viecap_build_prompt(self.h, ptr(cont.contiguous()) if cont is not None else None,
                                               ptr(tok) if tok is not None else None, N, Lt, 1 if soft_first else 0, ptr(out), _stream()))
        return out

    # ---- beam search building blocks (search.py:193-285): the W beams of ONE image are the rows of these calls
    def lm_prefill(self, embeds: torch.Tensor) -> torch.Tensor:
        """embeds [W, P, E] (the prompt, once per beam) -> log(softmax(next-token logits)) [W, vocab]."""
        embeds = self._dev(embeds).contiguous()
        W, P = int(embeds.shape[0]), int(embeds.shape[1])
        logp = torch.empty(W, self.cfg.dec_vocab, device=self.device, dtype=torch.float32)
        check(self.lib.pio_lm_prefill(self.h, ptr(embeds), W, P, ptr(logp), _stream()))
        return logp

    def lm_advance(self, tokens: torch.Tensor, src_rows: Optional[torch.Tensor], pos: int) -> torch.Tensor:
        """Row n continues the sequence of row src_rows[n] (None: as they are) with tokens[n] at position ``pos`` -> log-probabilities."""
        tok = self._dev(tokens, torch.int32).contiguous()
        src = self._dev(src_rows, torch.int32).contiguous() if src_rows is not None else None
        W = int(tok.shape[0])
        logp = torch.empty(W, self.cfg.dec_vocab, device=self.device, dtype=torch.float32)
        check(self.lib.pio_lm_advance(self.h, ptr(tok), ptr(src) if src is not None else None, W, int(pos), ptr(logp), _stream()))
        return logp

    def beam_select(self, logp: torch.Tensor, scores=None, lens=None, stopped=None):
        """One selection of beam_search (see pio_beam_select) -> (values [W] fp32, flat indices [W] int64), on the host."""
        W = int(logp.shape[0])
        val = torch.empty(W, device=self.device, dtype=torch.float32)
        idx = torch.empty(W, device=self.device, dtype=torch.int64)
        if scores is None:
            check(self.lib.pio_beam_select(self.h, ptr(logp), None, None, None, W, ptr(val), ptr(idx), _stream()))
        else:
            sc, ln = self._dev(scores, torch.float32).contiguous(), self._dev(lens, torch.float32).contiguous()
            st = self._dev(stopped, torch.int32).contiguous()
            check(self.lib.pio_beam_select(self.h, ptr(logp), ptr(sc), ptr(ln), ptr(st), W, ptr(val), ptr(idx), _stream()))
        return val.cpu(), idx.cpu()

    # ---- batched beam search: N images x W beams as the rows of one decode, the bookkeeping on the device (pio_lm_beam_search)
    def lm_beam_search(self, embeds: torch.Tensor, plen: Optional[torch.Tensor], beam_width: int, eos: Sequence[int], steps: int = 64):
        """embeds [N, Pmax, E] device (image n's prompt: its first plen[n] positions), plen [N] int32 device or None (all Pmax) ->
        (ids [N, W, steps] int32, lens [N, W] int32, scores [N, W] fp32) on the device, per image and beam in the order of the last
        selection; image n's are VieCapHead.beam_search's for it alone.  Enqueue-only; chunks of min(max_prefixes, 128) // W images."""
        embeds = self._dev(embeds).contiguous()
        W = int(beam_width)
        N, Pmax = int(embeds.shape[0]), int(embeds.shape[1])
        ids = torch.empty(N, W, steps, device=self.device, dtype=torch.int32)
        lens = torch.empty(N, W, device=self.device, dtype=torch.int32)
        scores = torch.empty(N, W, device=self.device, dtype=torch.float32)
        if plen is not None:
            plen = self._dev(plen, torch.int32).contiguous()
        chunk = max(1, min(self.max_prefixes, 128) // W)
        for s in range(0, N, chunk):
            e = min(N, s + chunk)
            check(self.lib.pio_lm_beam_search(self.h, ptr(embeds[s:e]), ptr(plen[s:e]) if plen is not None else None, e - s, Pmax, W,
                                              int(steps), int(eos[0]), int(eos[1]), ptr(ids[s:e]), ptr(lens[s:e]), ptr(scores[s:e]),
                                              _stream()))
        return ids, lens, scores

    def viecap_build_prompt_ragged(self, cont: Optional[torch.Tensor], tokens: Optional[torch.Tensor], lens: Optional[torch.Tensor],
                                   soft_first: bool = True):
        """The prompts of viecap_decode_ragged (pio_viecap_build_prompt_ragged): -> (prompt [N, Lc + Ltmax, E], plen [N] int32), device."""
        if cont is None and tokens is None:
            raise ValueError("viecap_build_prompt_ragged: neither a soft prompt nor prompt tokens")
        if (tokens is None) != (lens is None):
            raise ValueError("viecap_build_prompt_ragged: tokens and lens go together")
        N = int(cont.shape[0] if cont is not None else tokens.shape[0])
        Lt = int(tokens.shape[1]) if tokens is not None else 0
        Lc = int(cont.shape[1]) if cont is not None else 0
        prompt = torch.empty(N, Lc + Lt, self.cfg.dec_embd, device=self.device, dtype=torch.float32)
        plen = torch.empty(N, device=self.device, dtype=torch.int32)
        check(self.lib.pio_viecap_build_prompt_ragged(self.h, ptr(cont.contiguous()) if cont is not None else None,
                                                      ptr(tokens.contiguous()) if tokens is not None else None,
                                                      ptr(lens.contiguous()) if lens is not None else None, N, Lt,
                                                      1 if soft_first else 0, ptr(prompt), ptr(plen), _stream()))
        return prompt, plen

    def viecap_beam_ragged(self, cont: Optional[torch.Tensor], tokens: Optional[torch.Tensor], lens: Optional[torch.Tensor],
                           beam_width: int, eos: Sequence[int], soft_first: bool = True, steps: int = 64):
        """Beam search of every row of stage()'s (cont, tokens, lens), each at its own prompt length: lm_beam_search on the prompts of
        viecap_build_prompt_ragged."""
        prompt, plen = self.viecap_build_prompt_ragged(cont, tokens, lens, soft_first=soft_first)
        return self.lm_beam_search(prompt, plen, beam_width, eos, steps=steps)

    # ------------------------------------------------------------------ ClipCap head: MLP mapper, nucleus sampling, sampling loop
    def clipcap_mapping(self, feats: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """feats [N, C] -> prefix [N, Lp, E] (pio_clipcap_mapping); ``normalize``: rows L2-normalised first, on a copy."""
        feats = self._dev(feats).contiguous()
        N = int(feats.shape[0])
        Lp = int(self.lib.pio_clipcap_prefix_length(self.h))
        out = torch.empty(N, Lp, self.cfg.dec_embd, device=self.device, dtype=torch.float32)
        cap = min(self.max_prefixes, 128)
        for s in range(0, N, cap):
            e = min(N, s + cap)
            check(self.lib.pio_clipcap_mapping(self.h, ptr(feats[s:e]), e - s, 1 if normalize else 0, ptr(out[s:e]), _stream()))
        return out

    def nucleus_sample(self, scores: torch.Tensor, uniforms: torch.Tensor, temperature: float, top_p: float, stop_id: int,
                       active: Optional[torch.Tensor] = None):
        """One top-p draw per row of scores [N, vocab] (pio_nucleus_sample) -> (tokens [N], active [N], kept-set sizes [N]), int32, device."""
        scores, uniforms = self._dev(scores).contiguous(), self._dev(uniforms).contiguous()
        N = int(scores.shape[0])
        act = torch.ones(N, device=self.device, dtype=torch.int32) if active is None else self._dev(active, torch.int32).clone()
        tok = torch.empty(N, device=self.device, dtype=torch.int32)
        kept = torch.empty(N, device=self.device, dtype=torch.int32)
        check(self.lib.pio_nucleus_sample(self.h, ptr(scores), N, float(temperature), float(top_p), ptr(uniforms), int(stop_id), ptr(act),
                                          ptr(tok), ptr(kept), _stream()))
        return tok, act, kept

    def lm_sample(self, embeds: torch.Tensor, steps: int, temperature: float, top_p: float, stop_id: int, seed: int = 0,
                  uniforms: Optional[torch.Tensor] = None, rows_per_call: Optional[int] = None):
        """embeds [N, P, E] -> (ids [N, steps] int32, lens [N] int32) on the device (pio_lm_sample): enqueue-only.  ``uniforms`` [N, steps]
        or None: Philox under ``seed`` with counter (row, step, 0, 0), row counted over the WHOLE batch.  Calls of min(max_prefixes, 128)
        rows, or ``rows_per_call``; a batch that needs more than one call gets its uniforms from the host copy of the generator
        (pio_host_philox_uniforms), since a call counts its rows from 0 -- the ids do not depend on how the batch is split."""
        embeds = self._dev(embeds).contiguous()
        N, P = int(embeds.shape[0]), int(embeds.shape[1])
        ids = torch.empty(N, steps, device=self.device, dtype=torch.int32)
        lens = torch.empty(N, device=self.device, dtype=torch.int32)
        cap = min(self.max_prefixes, 128)
        if rows_per_call is not None:
            cap = max(1, min(cap, int(rows_per_call)))
        if uniforms is None and N > cap:
            uniforms = torch.empty(N, steps, dtype=torch.float32)
            check(self.lib.pio_host_philox_uniforms(int(seed) & 0xFFFFFFFFFFFFFFFF, 0, N, int(steps), ptr(uniforms)))
        if uniforms is not None:
            uniforms = self._dev(uniforms).contiguous()
        for s in range(0, N, cap):
            e = min(N, s + cap)
            check(self.lib.pio_lm_sample(self.h, ptr(embeds[s:e]), e - s, P, int(steps), float(temperature), float(top_p), int(stop_id),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(uniforms[s:e]) if uniforms is not None else None, ptr(ids[s:e]),
                                         ptr(lens[s:e]), _stream()))
        return ids, lens

    # ------------------------------------------------------------------ a11/a12 decoder
    def decode_greedy(self, prefix: torch.Tensor, steps: int = 30, want_logprob: bool = False, stop_id: Optional[int] = None,
                      seg: Optional[int] = None):
        """prefix [N, prefix_size] -> (greedy ids [N, steps] int32, per-token log-probabilities [N, steps] or None).

        ``stop_id`` (stop_at_eos; no log-probabilities): every chunk of max_prefixes rows runs in segments of ``seg`` steps (default
        DEFAULT_STOP_SEGMENT) and ends once each of its rows has emitted ``stop_id`` (pio_decode_greedy_stop: BLOCKING).  The ids are then
        the canonical table -- a row's first stop id repeated to the end of the row -- and ``last_steps_run`` lists the steps every chunk
        ran."""
        if stop_id is not None and want_logprob:
            raise ValueError("decode_greedy: a decode that stops early has no log-probabilities (the score sums all of them)")
        stops = _stop_ids(None if stop_id is None else [stop_id], 1)
        prefix = self._dev(prefix)
        N = prefix.shape[0]
        ids = torch.empty(N, steps, device=self.device, dtype=torch.int32)
        lp = torch.empty(N, steps, device=self.device, dtype=torch.float32) if want_logprob else None
        chunk = min(self.max_prefixes, 64) if want_logprob else self.max_prefixes     # the exact (log-prob) head: <= 64 rows
        ran = []
        for s in range(0, N, chunk):
            e = min(N, s + chunk)
            if stops is None:
                check(self.lib.pio_decode_greedy(self.h, ptr(prefix[s:e]), e - s, steps, ptr(ids[s:e]),
                                                 ptr(lp[s:e]) if want_logprob else None, _stream()))
                continue
            n = ctypes.c_int32(0)
            check(self.lib.pio_decode_greedy_stop(self.h, ptr(prefix[s:e]), e - s, steps, stops[0], _stop_seg(seg), ptr(ids[s:e]),
                                                  ctypes.byref(n), _stream()))
            ran.append(int(n.value))
        if stops is not None:
            self.last_steps_run = ran
        return ids, lp


class DecoderClone:
    """Handle from pio_clone_decoder: borrows the parent's decoder weights, owns its workspaces.  decode_greedy, viecap_decode_ragged and
    the batched beam search (the soft prompt and the token rows come from the parent: the mapping network and the entity table stay on it)."""

    def __init__(self, parent: Engine):
        self.lib, self.parent, self.device = parent.lib, parent, parent.device
        self.max_prefixes, self.max_steps, self.prefix_size = parent.max_prefixes, parent.max_steps, parent.prefix_size
        self.cfg = parent.cfg
        h = ctypes.c_void_p()
        check(self.lib.pio_clone_decoder(parent.h, ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.pio_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _dev = Engine._dev
    decode_greedy = Engine.decode_greedy
    viecap_decode_ragged = Engine.viecap_decode_ragged
    lm_beam_search = Engine.lm_beam_search
    viecap_build_prompt_ragged = Engine.viecap_build_prompt_ragged
    viecap_beam_ragged = Engine.viecap_beam_ragged
    lm_sample = Engine.lm_sample
