"""A minimal restatement of the PEFT LoRA layout on a host transformer (what `pipe.load_lora_weights(...)` leaves in `pipe.transformer`):
a wrapped Linear `X` becomes a `LoraLinear` with `X.base_layer`, `X.lora_A[adapter]` ([r, in]) / `X.lora_B[adapter]` ([out, r]) bias-free
Linears in ModuleDicts, `X.scaling[adapter]` (alpha / r times the set_adapters weight), `X.active_adapters`, `X.disable_adapters`,
`X.merged_adapters`, and the side-path forward `base(x) + sum scaling * B(A(x))`.  State-dict keys: `X.base_layer.weight`,
`X.base_layer.bias`, `X.lora_A.<adapter>.weight`, `X.lora_B.<adapter>.weight`.  peft itself is not installed in the build image
(tests/test_gpu_lora_adoption.py compares the names with a real injection where it is).  Test infrastructure only."""
import torch
import torch.nn as nn


class LoraLinear(nn.Module):
    def __init__(self, base_layer: nn.Module):
        super().__init__()
        self.base_layer = base_layer
        self.lora_A, self.lora_B, self.lora_dropout = nn.ModuleDict(), nn.ModuleDict(), nn.ModuleDict()
        self.lora_embedding_A, self.lora_embedding_B = nn.ParameterDict(), nn.ParameterDict()
        self.lora_magnitude_vector = nn.ModuleDict()
        self.r, self.lora_alpha, self.scaling, self.use_dora, self.lora_bias = {}, {}, {}, {}, {}
        self._active_adapter, self._disable_adapters, self.merged_adapters = [], False, []

    @property
    def active_adapters(self):
        return list(self._active_adapter)

    @property
    def disable_adapters(self):
        return self._disable_adapters

    @property
    def merged(self):
        return bool(self.merged_adapters)

    def update_layer(self, name, r, alpha, generator, std=0.05):
        out_f, in_f = self.base_layer.weight.shape[0], self.base_layer.weight.shape[-1]
        dtype = self.base_layer.weight.dtype
        self.lora_A[name], self.lora_B[name] = nn.Linear(in_f, r, bias=False), nn.Linear(r, out_f, bias=False)
        self.lora_dropout[name] = nn.Identity()
        with torch.no_grad():
            self.lora_A[name].weight.copy_(torch.randn(r, in_f, generator=generator) * std)
            self.lora_B[name].weight.copy_(torch.randn(out_f, r, generator=generator) * std)
        self.lora_A[name].to(dtype), self.lora_B[name].to(dtype)
        self.r[name], self.lora_alpha[name], self.scaling[name] = r, alpha, alpha / r
        self.use_dora[name], self.lora_bias[name] = False, False
        if name not in self._active_adapter:
            self._active_adapter.append(name)

    def forward(self, x, *a, **k):
        out = self.base_layer(x, *a, **k)
        if self.disable_adapters or self.merged:
            return out
        for name in self.active_adapters:
            if name in self.lora_A:
                out = out + self.lora_B[name](self.lora_A[name](self.lora_dropout[name](x.to(self.lora_A[name].weight.dtype)))).to(out.dtype) \
                    * self.scaling[name]
        return out


def layers(module):
    return {n: m for n, m in module.named_modules() if isinstance(m, LoraLinear)}


def _set(root, path, new):
    parent = root
    *head, leaf = path.split(".")
    for p in head:
        parent = getattr(parent, p)
    if isinstance(parent, (nn.ModuleList, nn.Sequential)) and leaf.isdigit():
        parent[int(leaf)] = new
    else:
        setattr(parent, leaf, new)


def inject(module, targets, rank, alpha, name, seed=0, std=0.05):
    """Wrap every sub-module whose path ends with one of `targets` (PEFT `target_modules` suffix matching; any module type - the adapter
    has to refuse what is not a Linear) and add adapter `name` of `rank` to it.  Returns the wrapped paths."""
    g = torch.Generator().manual_seed(seed)
    hit = []
    for path, m in list(module.named_modules()):
        if ".base_layer" in path or ".lora_" in path or not any(path == t or path.endswith("." + t) for t in targets):
            continue
        if not isinstance(m, LoraLinear):
            wrapped = LoraLinear(m)
            _set(module, path, wrapped)
            m = wrapped
        m.update_layer(name, rank, alpha, g, std)
        hit.append(path)
    return hit


def set_scale(module, name, weight):
    """`set_adapters(name, weight)`: scaling = alpha / r * weight on every layer that holds the adapter."""
    for m in layers(module).values():
        if name in m.scaling:
            m.scaling[name] = m.lora_alpha[name] / m.r[name] * weight


def disable(module, flag=True):
    for m in layers(module).values():
        m._disable_adapters = flag


def delete(module, name):
    for m in layers(module).values():
        for d in (m.lora_A, m.lora_B, m.lora_dropout, m.r, m.lora_alpha, m.scaling, m.use_dora, m.lora_bias):
            if name in d:
                del d[name]
        if name in m._active_adapter:
            m._active_adapter.remove(name)


def merged_weight(m):
    """fp32 `W + sum scaling * B A` of one wrapped layer's active adapters (what merge_adapter adds to the base weight)."""
    w = m.base_layer.weight.detach().float()
    if not m.disable_adapters and not m.merged:
        for name in m.active_adapters:
            w = w + m.scaling[name] * (m.lora_B[name].weight.detach().float() @ m.lora_A[name].weight.detach().float())
    return w


def merge(module):
    """`merge_adapter()` / `fuse_lora()`: the active adapters go into base_layer.weight (on the CPU, in the weight's dtype) and are listed
    in `merged_adapters`; the side path is then off."""
    for m in layers(module).values():
        w = merged_weight(m)
        with torch.no_grad():
            m.base_layer.weight.copy_(w.to(m.base_layer.weight.dtype))
        m.merged_adapters = list(m.active_adapters)


def unload(module):
    """`unload_lora_weights()`: every wrapper is replaced by its base layer."""
    for path, m in list(layers(module).items()):
        _set(module, path, m.base_layer)
