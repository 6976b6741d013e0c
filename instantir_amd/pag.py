"""Perturbed-attention guidance (PAG, Ahn et al. 2024, arXiv 2403.17377): host-side rules.

The behaviour follows diffusers' PAG pipelines (processor `PAGCFGIdentitySelfAttnProcessor2_0`, guidance
`_apply_perturbed_attention_guidance`), which came after the pinned diffusers 0.28.1; DESIGN.md section 7 states the contract.
This module holds what needs no GPU: which self-attention modules a layer list selects, and the per-step scale s_t."""
from __future__ import annotations

import re
from typing import Iterable, List, Sequence, Union

DEFAULT_PAG_SCALE = 3.0          # diffusers' default when a PAG pipeline is called without pag_scale


def attn1_paths(cfg) -> List[str]:
    """Dotted diffusers module names of every self-attention (`attn1`) of the main UNet, in forward order."""
    out = []
    for i, d in enumerate(cfg.transformer_depth):
        for j in range(cfg.layers_per_block if d > 0 else 0):
            out += [f"down_blocks.{i}.attentions.{j}.transformer_blocks.{k}.attn1" for k in range(d)]
    out += [f"mid_block.attentions.0.transformer_blocks.{k}.attn1" for k in range(cfg.mid_depth)]
    for i, d in enumerate(reversed(cfg.transformer_depth)):
        for j in range(cfg.layers_per_block + 1 if d > 0 else 0):
            out += [f"up_blocks.{i}.attentions.{j}.transformer_blocks.{k}.attn1" for k in range(d)]
    return out


def normalize_layers(layers: Union[str, Sequence[str]], what: str = "pag_applied_layers") -> List[str]:
    if isinstance(layers, str):
        layers = [layers]
    layers = list(layers)
    if not layers:
        raise ValueError(f"{what} is empty: name at least one layer (e.g. 'mid')")
    for e in layers:
        if not isinstance(e, str) or not e:
            raise ValueError(f"{what} entries must be non-empty strings, got {e!r}")
    return layers


def select(layers: Union[str, Sequence[str]], paths: Iterable[str], what: str = "pag_applied_layers") -> List[str]:
    """The `attn1` paths selected by `layers`: each entry is a regular expression, and a path is selected when it contains a
    match of it that ends at a '.', at a '_' or at the end of the name ('down_blocks.1' never selects 'down_blocks.10...',
    'blocks.1' never 'blocks.10', 'up_blocks.0.att' nothing; '_' lets 'mid' select 'mid_block...').  An entry that selects
    nothing, or an empty list, raises ValueError naming it (and `what`, the argument the list came from)."""
    layers = normalize_layers(layers, what)
    paths = list(paths)
    chosen = set()
    for e in layers:
        try:
            rx = re.compile(f"(?:{e})(?=[._]|$)")
        except re.error as err:
            raise ValueError(f"{what} entry {e!r} is not a regular expression: {err}") from None
        hit = [p for p in paths if rx.search(p)]
        if not hit:
            raise ValueError(f"{what} entry {e!r} selects no self-attention layer of the UNet")
        chosen.update(hit)
    return [p for p in paths if p in chosen]


def scale_at(pag_scale: float, pag_adaptive_scale: float, t: float) -> float:
    """s_t = max(pag_scale - pag_adaptive_scale * (1000 - t), 0), t the timestep the UNet sees (fractional for Karras)."""
    s = float(pag_scale)
    if pag_adaptive_scale:
        s = s - float(pag_adaptive_scale) * (1000.0 - float(t))
    return max(s, 0.0)


def check_engine(net) -> None:
    """PAG needs the fp16 self-attention path: a UNet built with fp8 linears is refused."""
    if getattr(net, "fp8_linear", False):
        raise ValueError("enable_pag: this UNet was built with fp8 linears (fp8_linear=True); perturbed-attention guidance "
                         "runs on the fp16 engine only")
