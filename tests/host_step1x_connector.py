"""Stand-in for the [EXT] `Qwen2Connector` of the public Step1X-Edit transformer (`transformer.connector`): the module the reference
calls once per CFG branch per computed step as `self.connector(x, t, mask)` (Step1XEdit/inplace.py:514-516,
Step1XEditV1P2/inplace.py:602-609).  Its class lives in a diffusers fork that is not installable here, so the PUBLIC LAYOUT is restated
as plain `nn.Module`s with the fork's parameter names (`regione_amd/step1x_connector.py` keeps the same names in one table):

    S.input_embedder                                   Linear(in, h)
    S.t_embedder.mlp.{0,2}                             Linear(256, h), SiLU, Linear(h, h) on cat(cos, sin)(t f), f = exp(-ln 1e4 arange(128) / 128)
    S.c_embedder.linear_1 / linear_2                   Linear(in, h), SiLU, Linear(h, h)
    S.individual_token_refiner.blocks.{i}.norm1/norm2  LayerNorm(h, eps 1e-6, affine)
                                  .self_attn_qkv       Linear(h, 3 h), columns (q | k | v)(head)(128)
                                  .self_attn_q_norm / self_attn_k_norm   RMSNorm(128, eps 1e-6)
                                  .self_attn_proj      Linear(h, h)
                                  .mlp.fc1 / fc2       Linear(h, 4 h), SiLU, Linear(4 h, h)
                                  .adaLN_modulation.1  SiLU, Linear(h, 2 h) -> gate_msa | gate_mlp
    global_proj_out                                    Linear(in, pooled)
    scale_factor                                       [1], init -0.91

Test infrastructure only."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

HEAD_DIM = 128


class RMSNorm(nn.Module):
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + self.eps)).type_as(x) * self.weight


class TimestepEmbedder(nn.Module):
    def __init__(self, hidden_size, frequency_embedding_size=256):
        super().__init__()
        self.frequency_embedding_size = frequency_embedding_size
        self.mlp = nn.Sequential(nn.Linear(frequency_embedding_size, hidden_size), nn.SiLU(), nn.Linear(hidden_size, hidden_size))

    def forward(self, t):
        half = self.frequency_embedding_size // 2
        f = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
        a = t[:, None].float() * f[None]
        emb = torch.cat([torch.cos(a), torch.sin(a)], dim=-1)
        return self.mlp(emb.to(self.mlp[0].weight.dtype))


class TextProjection(nn.Module):
    def __init__(self, in_channels, hidden_size):
        super().__init__()
        self.linear_1 = nn.Linear(in_channels, hidden_size)
        self.act_1 = nn.SiLU()
        self.linear_2 = nn.Linear(hidden_size, hidden_size)

    def forward(self, x):
        return self.linear_2(self.act_1(self.linear_1(x)))


class MLP(nn.Module):
    def __init__(self, hidden_size, mlp_hidden):
        super().__init__()
        self.fc1 = nn.Linear(hidden_size, mlp_hidden)
        self.act = nn.SiLU()
        self.fc2 = nn.Linear(mlp_hidden, hidden_size)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class IndividualTokenRefinerBlock(nn.Module):
    def __init__(self, hidden_size, heads_num):
        super().__init__()
        self.heads_num = heads_num
        self.norm1 = nn.LayerNorm(hidden_size, elementwise_affine=True, eps=1e-6)
        self.self_attn_qkv = nn.Linear(hidden_size, 3 * hidden_size)
        self.self_attn_q_norm = RMSNorm(hidden_size // heads_num)
        self.self_attn_k_norm = RMSNorm(hidden_size // heads_num)
        self.self_attn_proj = nn.Linear(hidden_size, hidden_size)
        self.norm2 = nn.LayerNorm(hidden_size, elementwise_affine=True, eps=1e-6)
        self.mlp = MLP(hidden_size, 4 * hidden_size)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(hidden_size, 2 * hidden_size))

    def forward(self, x, c, attn_mask):
        gate_msa, gate_mlp = self.adaLN_modulation(c).chunk(2, dim=1)
        B, L, _ = x.shape
        qkv = self.self_attn_qkv(self.norm1(x)).view(B, L, 3, self.heads_num, -1)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))                      # [B, H, L, D]
        q, k = self.self_attn_q_norm(q), self.self_attn_k_norm(k)
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask).transpose(1, 2).reshape(B, L, -1)
        x = x + self.self_attn_proj(a) * gate_msa[:, None]
        return x + self.mlp(self.norm2(x)) * gate_mlp[:, None]


class IndividualTokenRefiner(nn.Module):
    def __init__(self, hidden_size, heads_num, depth):
        super().__init__()
        self.blocks = nn.ModuleList([IndividualTokenRefinerBlock(hidden_size, heads_num) for _ in range(depth)])

    def forward(self, x, c, mask):
        B, L, _ = x.shape
        m = mask.to(torch.bool)
        A = (m[:, None, :, None] & m[:, None, None, :]).clone()                         # [B, 1, L, L]: A[i, j] = mask[i] & mask[j]
        A[:, :, :, 0] = True                                                            # padded query rows see key 0 only
        for blk in self.blocks:
            x = blk(x, c, A)
        return x


class SingleTokenRefiner(nn.Module):
    def __init__(self, in_channels, hidden_size, heads_num, depth):
        super().__init__()
        self.input_embedder = nn.Linear(in_channels, hidden_size)
        self.t_embedder = TimestepEmbedder(hidden_size)
        self.c_embedder = TextProjection(in_channels, hidden_size)
        self.individual_token_refiner = IndividualTokenRefiner(hidden_size, heads_num, depth)

    def forward(self, x, t, mask, mean):
        c = self.t_embedder(t) + self.c_embedder(mean)
        return self.individual_token_refiner(self.input_embedder(x), c, mask)


class Qwen2Connector(nn.Module):
    def __init__(self, in_channels=3584, hidden_size=4096, heads_num=32, depth=2, pooled_dim=768):
        super().__init__()
        self.S = SingleTokenRefiner(in_channels, hidden_size, heads_num, depth)
        self.global_proj_out = nn.Linear(in_channels, pooled_dim)
        self.scale_factor = nn.Parameter(torch.zeros(1) - 0.91)

    def forward(self, x, t, mask):
        m = mask[..., None].to(x.dtype)
        mean = (x * m).sum(1) / m.sum(1)
        y = self.global_proj_out(mean * (1 + self.scale_factor))
        return self.S(x, t, mask, mean), y


def make_connector(in_channels, hidden_size, heads_num, depth=2, pooled_dim=64, seed=0, dtype=torch.bfloat16):
    """The stand-in with the weights the parity tests use: N(0, 1 / fan_in) matrices, norm weights 1 +- 0.1, biases 0.02 N(0, 1)."""
    mod = Qwen2Connector(in_channels, hidden_size, heads_num, depth, pooled_dim)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n == "scale_factor":
                continue
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p.shape[1]))
            elif n.endswith("bias"):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
    return mod.to(dtype)
