"""HarmonicEmbedding: the positional encoding in front of a NeRF-style MLP, on csrc/harmonic.hip, forward and backward.

    harmonic_embedding(x, frequencies, diag_cov=None, append_input=True) -> (..., dim (2 n + append_input))
    harmonic_embedding_torch(...)      the reference's chain restated: any dtype and device
    HarmonicEmbedding(n_harmonic_functions=6, omega_0=1.0, logspace=True, append_input=True)    the reference's module

The reference (pytorch3d/renderer/implicit/harmonic_embedding.py) multiplies x into (..., dim, n), adds [0, pi/2] into (..., 2, dim, n),
takes sin, reshapes (a copy) and concatenates with x: about four tensors of the output's size are written and read again, and autograd
keeps one for a backward that walks the chain once more.  Here float32 GPU tensors are ONE autograd node: the forward reads dim floats
and writes dim (2 n + 1) per row, the backward reads the output's gradient once and writes dim floats per row, and nothing but x (and
diag_cov) is kept between the two.  The backward has no atomics: the same bits on every run and stream, with or without
torch.use_deterministic_algorithms.

Contract: csrc/implicit_abi.h -- the reference's formula, operation for operation: t = x f and a = t + [0, float32(pi / 2)] are two
float32 roundings, the cos block is sin(t + pi/2) and not cos(t), with diag_cov the factor is exp(-0.5 (diag_cov (f f))).  `frequencies`
is the module's `_frequencies` buffer (omega_0 already multiplied in) with any values.

Everything else -- CPU tensors, float64 / half, a diag_cov that broadcasts, n = 0, frequencies that require grad, rows wider than
the backward's LDS tile or outputs beyond 32-bit indices -- takes `harmonic_embedding_torch`, differentiated by autograd.
"""
import math

import torch

from . import _C

CALLS = {"fused": 0, "chain": 0}  # what ran (the shim's PATCH_CALLS and the tests read it)

HALF_PI = 0.5 * math.pi  # rounded to float32 where it meets float32 data, as the reference's _zero_half_pi buffer is


def harmonic_embedding_torch(x, frequencies, diag_cov=None, append_input=True, zero_half_pi=None):
    """The reference's HarmonicEmbedding.forward (harmonic_embedding.py:140-158) on a frequencies tensor.  zero_half_pi: the module's
    buffer; None makes it in float32 and casts to x's dtype (what `.double()` of the module does to the buffer)."""
    if zero_half_pi is None:
        zero_half_pi = torch.tensor([0.0, HALF_PI], dtype=torch.float32, device=x.device).to(x.dtype if x.is_floating_point() else torch.float32)
    embed = x[..., None] * frequencies
    embed = embed[..., None, :, :] + zero_half_pi[..., None, None]
    embed = embed.sin()
    if diag_cov is not None:
        x_var = diag_cov[..., None] * torch.pow(frequencies, 2)
        exp_var = torch.exp(-0.5 * x_var)
        embed = embed * exp_var[..., None, :, :]
    embed = embed.reshape(*x.shape[:-1], 2 * x.shape[-1] * frequencies.shape[0])  # (the reference's -1 refuses an input of 0 rows)
    if append_input:
        return torch.cat([embed, x], dim=-1)
    return embed


def kernel_path(x, frequencies, diag_cov=None, append_input=True):
    """Whether harmonic_embedding(...) of these inputs runs csrc/harmonic.hip's kernels (else: the reference's chain restated).  Decided
    by dtypes, devices and shape arithmetic alone."""
    tensors = [x, frequencies] + ([] if diag_cov is None else [diag_cov])
    if not all(torch.is_tensor(t) for t in tensors):
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.device == x.device for t in tensors):
        return False
    if x.dim() < 1 or frequencies.dim() != 1 or frequencies.requires_grad:
        return False
    if diag_cov is not None and diag_cov.shape != x.shape:
        return False
    dim, n = x.shape[-1], frequencies.shape[0]
    rows = math.prod(x.shape[:-1])
    return _C.harmonic_embedding_fits(rows, dim, n, append_input)


class _HarmonicEmbedding(torch.autograd.Function):
    """out (rows, W) of x (rows, dim), diag_cov (rows, dim) or None and frequencies (n,)."""

    @staticmethod
    def forward(ctx, x, diag_cov, frequencies, append_input):
        ctx.append_input = append_input
        saved = [x.detach(), None if diag_cov is None else diag_cov.detach(), frequencies.detach()]
        ctx.save_for_backward(*saved)
        return _C.harmonic_embedding_forward(saved[0], saved[1], saved[2], append_input)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, diag_cov, frequencies = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gc = _C.harmonic_embedding_backward(x, diag_cov, frequencies, grad_out, ctx.append_input, need[0], need[1])
        return gx, gc, None, None


def harmonic_embedding(x, frequencies, diag_cov=None, append_input: bool = True):
    """See the module docstring."""
    if not kernel_path(x, frequencies, diag_cov, append_input):
        CALLS["chain"] += 1
        return harmonic_embedding_torch(x, frequencies, diag_cov, append_input)
    CALLS["fused"] += 1
    lead, dim = tuple(x.shape[:-1]), x.shape[-1]
    # a non-contiguous x (or diag_cov) is copied: 1 / (2 n + 1) of the output
    out = _HarmonicEmbedding.apply(x.reshape(-1, dim).contiguous(), None if diag_cov is None else diag_cov.reshape(-1, dim).contiguous(),
                                   frequencies.contiguous(), bool(append_input))
    return out.view(lead + (out.shape[-1],))


class HarmonicEmbedding(torch.nn.Module):
    """The reference's module: its constructor, its two non-persistent buffers, `forward(x, diag_cov=None, **kwargs)` and the two
    output-size helpers; forward is `harmonic_embedding` above."""

    def __init__(self, n_harmonic_functions: int = 6, omega_0: float = 1.0, logspace: bool = True, append_input: bool = True) -> None:
        super().__init__()
        if logspace:
            frequencies = 2.0 ** torch.arange(n_harmonic_functions, dtype=torch.float32)
        else:
            frequencies = torch.linspace(1.0, 2.0 ** (n_harmonic_functions - 1), n_harmonic_functions, dtype=torch.float32)
        self.register_buffer("_frequencies", frequencies * omega_0, persistent=False)
        self.register_buffer("_zero_half_pi", torch.tensor([0.0, 0.5 * torch.pi]), persistent=False)
        self.append_input = append_input

    def forward(self, x: torch.Tensor, diag_cov=None, **kwargs) -> torch.Tensor:
        return module_forward(self, x, diag_cov)

    @staticmethod
    def get_output_dim_static(input_dims: int, n_harmonic_functions: int, append_input: bool) -> int:
        return input_dims * (2 * n_harmonic_functions + int(append_input))

    def get_output_dim(self, input_dims: int = 3) -> int:
        return self.get_output_dim_static(input_dims, len(self._frequencies), self.append_input)


def module_path(module, x, diag_cov=None):
    """kernel_path for a module of the reference's layout, by its buffers as they are now: `.double()` or `.half()` of the module go
    to the chain.  The kernels hold float32(pi / 2) as a constant: the buffer's dtype and shape are checked, its values are not."""
    zhp = module._zero_half_pi
    return (kernel_path(x, module._frequencies, diag_cov, module.append_input) and zhp.dtype == torch.float32 and zhp.device == x.device
            and tuple(zhp.shape) == (2,))


def module_forward(module, x, diag_cov=None):
    """forward of a module with the reference's buffers (`_frequencies`, `_zero_half_pi`) and `append_input`: this package's class and,
    through the shim, the reference's own."""
    if module_path(module, x, diag_cov):
        return harmonic_embedding(x, module._frequencies, diag_cov, module.append_input)
    CALLS["chain"] += 1
    return harmonic_embedding_torch(x, module._frequencies, diag_cov, module.append_input, zero_half_pi=module._zero_half_pi)
