"""Float64 statements of the ViT block kernels (csrc/vit_gemm*.hip, vit_attention.hip, text_encoder.hip, vit_misc.hip), for
tests/test_gpu_vit_kernels.py.  No test functions here.

Every function takes the SAME rounded operands the kernel gets (fp16 / bf16 tensors, fp32 epilogue operands) and computes in float64 on
whatever device they live on (the large cases run their matmuls on the GPU).  The layouts are the kernels' (kernels.h, GemmEpilogue)."""
import math
from typing import Optional, Sequence

import torch

from viecap_ref64 import layer_norm64  # noqa: F401  (the same two-pass statement serves the ViT LayerNorm)

F64 = torch.float64


def gemm64(A: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """A [M][K] . W [N][K]^T."""
    return A.to(F64) @ W.to(F64).t()


def mag64(A: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """sum over k of |A[m][k]| |W[n][k]|: the magnitude an accumulated rounding error is proportional to."""
    return A.to(F64).abs() @ W.to(F64).abs().t()


def gelu_erf64(v: torch.Tensor) -> torch.Tensor:
    """0.5 v (1 + erf(v / sqrt 2)), the exact-erf GELU of DINOv2's MLP."""
    v = v.to(F64)
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def quick_gelu64(v: torch.Tensor) -> torch.Tensor:
    """v sigmoid(1.702 v), the OpenAI-CLIP activation."""
    v = v.to(F64)
    return v * torch.sigmoid(1.702 * v)


def patch_embed64(acc: torch.Tensor, bias: torch.Tensor, pos: torch.Tensor, n2: int, Tp: int, G: int) -> torch.Tensor:
    """acc [B n2][D] -> the rows b Tp + G + p of x [B Tp][D] (other rows NaN: the kernel does not write them)."""
    B = acc.shape[0] // n2
    D = acc.shape[1]
    x = torch.full((B * Tp, D), float("nan"), dtype=F64, device=acc.device)
    v = acc.to(F64) + bias.to(F64) + pos[1:1 + n2].to(F64).repeat(B, 1)
    rows = (torch.arange(B, device=acc.device)[:, None] * Tp + G + torch.arange(n2, device=acc.device)[None]).reshape(-1)
    x[rows] = v
    return x


def qkv_split64(C: torch.Tensor, B: int, Tp: int, Tk: int, H: int):
    """C [B Tp][3D] (bias included) -> q, k [B][H][Tk][64] and vT [B][H][64][Tk] (token slots >= Tp NaN: not written)."""
    D = C.shape[1] // 3
    c = C.to(F64).reshape(B, Tp, 3, H, 64)
    q = torch.full((B, H, Tk, 64), float("nan"), dtype=F64, device=C.device)
    k = q.clone()
    vT = torch.full((B, H, 64, Tk), float("nan"), dtype=F64, device=C.device)
    q[:, :, :Tp] = c[:, :, 0].permute(0, 2, 1, 3)
    k[:, :, :Tp] = c[:, :, 1].permute(0, 2, 1, 3)
    vT[:, :, :, :Tp] = c[:, :, 2].permute(0, 2, 3, 1)
    assert D == 64 * H
    return q, k, vT


def capture64(C: torch.Tensor, B: int, Tp: int, T: int) -> torch.Tensor:
    """The fp32 capture of the last block's qkv: [B][T][3D], rows t < T of every image."""
    return C.to(F64).reshape(B, Tp, -1)[:, :T]


def residual64(A: torch.Tensor, Wf: torch.Tensor, x: torch.Tensor, bf: torch.Tensor) -> torch.Tensor:
    """x + A (ls W)^T + ls b with LayerScale already folded into the operands (Wf, bf), as the kernels get them."""
    return x.to(F64) + gemm64(A, Wf) + bf.to(F64)


def attention64(q: torch.Tensor, k: torch.Tensor, vT: torch.Tensor, scale: float, T: int, lens: Optional[Sequence[int]] = None,
                causal: bool = False) -> torch.Tensor:
    """softmax(scale q k^T) v per (image, head) over the keys < lens[b] (or all T; causal: keys <= the query).  q, k [B][H][Tk][64],
    vT [B][H][64][Tk] -> [B][H][T][64] for the queries t < T."""
    B, H = q.shape[:2]
    out = []
    for b in range(B):
        n = T if lens is None else int(lens[b])
        qb = q[b, :, :T].to(F64)
        kb = k[b, :, :T].to(F64)
        vb = vT[b, :, :, :T].to(F64).transpose(1, 2)
        s = scale * (qb @ kb.transpose(1, 2))
        mask = torch.zeros(T, T, dtype=torch.bool, device=q.device)
        mask[:, n:] = True
        if causal:
            mask |= torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
        out.append(torch.softmax(s, -1) @ vb)
    return torch.stack(out)
