"""The three error measures of ``ppq/quantization/measure/`` (norm.py, cosine.py) with the reference's signatures.

float32 contiguous tensors on the GPU that record no gradient go through the kernels of ``csrc/measure.hip``: one streaming
read of both tensors gives the four row sums (noise, signal, pp, pr) in double, a second tiny launch turns them into the
per-row measure in fp32.  Everything else -- CPU tensors, other dtypes, tensors that require grad -- takes the reference's
torch expressions, restated below.

(``blocks.torch_mean_square_error`` is the training loss of the finetuning passes and stays what it is.)
"""
import torch

_REDUCTIONS = ('mean', 'sum', 'none')


def _prepare(y_pred: torch.Tensor, y_real: torch.Tensor, what: str, reduction: str):
    if y_pred.shape != y_real.shape:
        raise ValueError(f'Can not compute {what} loss for tensors with different shape. '
                         f'({y_pred.shape} and {y_real.shape})')
    reduction = str(reduction).lower()
    if y_pred.ndim == 1:
        y_pred, y_real = y_pred.unsqueeze(0), y_real.unsqueeze(0)
    return y_pred, y_real, reduction


def _reduce(rows: torch.Tensor, reduction: str) -> torch.Tensor:
    if reduction == 'mean': return torch.mean(rows)
    if reduction == 'sum': return torch.sum(rows)
    if reduction == 'none': return rows
    raise ValueError('Unsupported reduction method.')


def reference_formula(method: str, y_pred: torch.Tensor, y_real: torch.Tensor, reduction: str = 'mean') -> torch.Tensor:
    """The reference's torch expressions for rows of ``[batch, ...]`` tensors of one shape, on whatever device they are."""
    y_pred, y_real = y_pred.flatten(start_dim=1), y_real.flatten(start_dim=1)
    if method == 'mse':
        rows = torch.mean(torch.pow(y_pred - y_real, 2), dim=-1)
    elif method == 'snr':
        noise_power = torch.pow(y_pred - y_real, 2).sum(dim=-1)
        signal_power = torch.pow(y_real, 2).sum(dim=-1)
        rows = noise_power / (signal_power + 1e-7)
    elif method == 'cosine':
        rows = torch.cosine_similarity(y_pred.float(), y_real.float(), dim=-1)
    else:
        raise ValueError(f'Unknown measure {method}: mse, snr and cosine exist.')
    return _reduce(rows, reduction)


def kernel_path(y_pred: torch.Tensor, y_real: torch.Tensor) -> bool:
    """Whether this pair is measured by the HIP kernels (see the module docstring)."""
    return (y_pred.is_cuda and y_real.is_cuda and y_pred.device == y_real.device
            and y_pred.dtype is torch.float32 and y_real.dtype is torch.float32
            and y_pred.is_contiguous() and y_real.is_contiguous() and y_pred.numel() > 0
            and not (torch.is_grad_enabled() and (y_pred.requires_grad or y_real.requires_grad)))


def _kernel_rows(y_pred: torch.Tensor, y_real: torch.Tensor, method: str) -> torch.Tensor:
    from . import ffi
    sums = ffi.measure_rows_multi([(y_pred, y_real, None)])[0]
    rows = torch.empty(y_pred.shape[0], dtype=torch.float32, device=y_pred.device)
    ffi.measure_finish_multi([(sums, y_pred.numel() // y_pred.shape[0], None, rows)], method)
    return rows


def torch_mean_square_error(y_pred: torch.Tensor, y_real: torch.Tensor, reduction: str = 'mean') -> torch.Tensor:
    """measure/norm.py:3-52: per sample mean((pred - real)^2), then the reduction over the batch."""
    y_pred, y_real, reduction = _prepare(y_pred, y_real, 'mse', reduction)
    if reduction not in _REDUCTIONS: raise ValueError('Unsupported reduction method.')
    if kernel_path(y_pred, y_real): return _reduce(_kernel_rows(y_pred, y_real, 'mse'), reduction)
    return reference_formula('mse', y_pred, y_real, reduction)


def torch_snr_error(y_pred: torch.Tensor, y_real: torch.Tensor, reduction: str = 'mean') -> torch.Tensor:
    """measure/norm.py:54-99: per sample sum((pred - real)^2) / (sum(real^2) + 1e-7)."""
    y_pred, y_real, reduction = _prepare(y_pred, y_real, 'snr', reduction)
    if reduction not in _REDUCTIONS: raise ValueError('Unsupported reduction method.')
    if kernel_path(y_pred, y_real): return _reduce(_kernel_rows(y_pred, y_real, 'snr'), reduction)
    return reference_formula('snr', y_pred, y_real, reduction)


def torch_cosine_similarity(y_pred: torch.Tensor, y_real: torch.Tensor, reduction: str = 'mean') -> torch.Tensor:
    """measure/cosine.py:6-29: per sample torch.cosine_similarity of the flattened tensors (the reference's message says
    'mse' here too)."""
    y_pred, y_real, reduction = _prepare(y_pred, y_real, 'mse', reduction)
    if reduction not in _REDUCTIONS: raise ValueError('Unsupported reduction method.')
    if kernel_path(y_pred, y_real): return _reduce(_kernel_rows(y_pred, y_real, 'cosine'), reduction)
    return reference_formula('cosine', y_pred, y_real, reduction)


def torch_cosine_similarity_as_loss(y_pred: torch.Tensor, y_real: torch.Tensor, reduction: str = 'mean') -> torch.Tensor:
    """measure/cosine.py:37-39."""
    return 1 - torch_cosine_similarity(y_pred=y_pred, y_real=y_real, reduction=reduction)
