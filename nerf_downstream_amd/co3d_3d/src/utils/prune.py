"""Pruning utilities (counterpart of the reference's co3d_3d/src/utils/prune.py:11-76), on torch.nn.utils.prune.

The reference's pruning trainer is not in its tree; `global_magnitude_prune` is the one step of it that the tests and the
benchmark need to make a pruned network."""
import torch.nn.utils.prune as torch_prune

from nerf_downstream_amd import minkowski as _HIP_ME


def count_parameters(model):
    """{"total": trainable parameters, "pruned": zeros of every `kernel_mask` / `weight_mask` buffer} (reference :11-22)."""
    return {
        "total": float(sum(p.numel() for p in model.parameters() if p.requires_grad)),
        "pruned": float(sum((1 - b.int()).sum() for n, b in model.named_buffers() if "kernel_mask" in n or "weight_mask" in n)),
    }


def count_flops(model):
    """GFLOP of the last forward pass: the sum of the `_flops` the weight-sparse layers left behind (reference :25-31).  One
    host read-back, here -- the layers keep their counts on the device."""
    flops = 0
    for _, module in model.named_modules():
        f = getattr(module, "_flops", None)
        if f is not None:
            flops = flops + f
    return float(flops) / 1e9


def get_parameters_to_prune(model, ME=None):
    """[(module, parameter name)]: the kernel of every convolution and transposed convolution, dense or weight-sparse (the
    weight-sparse classes derive from the dense ones), and `linear.weight` of every MinkowskiLinear (reference :34-57)."""
    ME = ME or getattr(model, "_ME", None) or _HIP_ME
    out = []
    for _, module in model.named_modules():
        if isinstance(module, (ME.MinkowskiConvolution, ME.MinkowskiConvolutionTranspose)):
            out.append((module, "kernel"))
        elif isinstance(module, ME.MinkowskiLinear):
            out.append((module.linear, "weight"))
    return out


def register_prune_buffers(parameters_to_prune):
    """Identity-prune: every parameter gets its `_orig` / `_mask` pair, so a pruned checkpoint loads (reference :60-62)."""
    for module, name in parameters_to_prune:
        torch_prune.identity(module, name)


def masks_and_parameters(parameters_to_prune):
    for module, name in parameters_to_prune:
        assert hasattr(module, f"{name}_mask"), f"module {module} has no attribute with name {name}_mask"
        assert hasattr(module, name), f"module {module} has no attribute with name {name}"
        yield getattr(module, f"{name}_mask"), getattr(module, f"{name}_orig")


def remove(parameters_to_prune):
    """Make the pruned state permanent: the zeros go into the parameter, the `_orig` / `_mask` pair is dropped."""
    for module, name in parameters_to_prune:
        torch_prune.remove(module, name)


def global_magnitude_prune(model, amount, ME=None):
    """Global unstructured L1 pruning of `amount` (a fraction, or a count) of the prunable weights -> the (module, name) list."""
    params = get_parameters_to_prune(model, ME=ME)
    torch_prune.global_unstructured(params, pruning_method=torch_prune.L1Unstructured, amount=amount)
    return params
