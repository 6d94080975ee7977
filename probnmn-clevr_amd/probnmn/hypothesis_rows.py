"""The layout of hypothesis rows, stated once: R program hypotheses of G questions lie in ``question_rows`` [R] order --
non-decreasing, in 0 .. G - 1; hypothesis r belongs to question ``question_rows[r]`` and a question may have none -- which
is what ``group_hypotheses`` returns and what ``pnmn_answer_marginal``, ``pnmn_hypothesis_posterior`` and
``pnmn_answer_posterior`` read as ``group_start`` [G + 1]: question g owns rows group_start[g] .. group_start[g + 1].
``NeuralModuleNetwork.marginal_answers`` / ``answer_posterior`` and ``evaluators.hypothesis_posterior`` take their arguments
through here.  Only ``group_start_on_device`` and ``row_vector`` touch a device."""
import numpy as np
import torch

from probnmn import _hip


def on_host(question_rows) -> np.ndarray:
    """``question_rows`` (a sequence, an array, a host or device tensor) as a contiguous host int64 array."""
    return np.ascontiguousarray(torch.as_tensor(question_rows).detach().cpu().numpy(), dtype=np.int64)


def check(qrows: np.ndarray, n_groups: int) -> None:
    """``ValueError`` unless the host rows [R] are non-decreasing and in 0 .. n_groups - 1."""
    if qrows.size and (int(qrows.min()) < 0 or int(qrows.max()) >= n_groups or bool((np.diff(qrows) < 0).any())):
        raise ValueError("question_rows must be non-decreasing and in 0 .. %d" % (n_groups - 1))


def group_start(qrows: np.ndarray, n_groups: int) -> np.ndarray:
    """Host int64 [n_groups + 1]: question g owns rows group_start[g] .. group_start[g + 1] of checked ``qrows``."""
    return np.searchsorted(qrows, np.arange(n_groups + 1))


def group_start_on_device(qrows: np.ndarray, n_groups: int, device: torch.device) -> torch.Tensor:
    """``group_start`` as the kernels read it: int32 [n_groups + 1] on the device, uploaded without a synchronisation."""
    return _hip.small_to_device(group_start(qrows, n_groups).tolist(), torch.int32, device)


def row_vector(values, name: str, n_rows: int, device: torch.device) -> torch.Tensor:
    """One number per hypothesis row (``log_weights``, ``log_q``) as contiguous fp32 [n_rows] on the device."""
    vector = torch.as_tensor(values).detach().to(device=device, dtype=torch.float32).contiguous()
    if tuple(vector.shape) != (n_rows,):
        raise ValueError("%s [%d]; got %s" % (name, n_rows, tuple(vector.shape)))
    return vector
