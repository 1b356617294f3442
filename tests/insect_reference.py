"""CPU restatement of the INSECT / BZSL arithmetic that tests/test_insect_cpu.py and tests/test_insect_gpu.py compare with: the class means
in numpy's row order, the CSV text of the prototype table, and the stable descending sort behind the logits' top-k."""
import io

import numpy as np
import torch


def class_mean(x: np.ndarray, labels: np.ndarray, num_classes: int):
    """(mean float32 [C, D], count int32 [C], error): for class c with rows i1 < i2 < ... the float32 chain ((x[i1] + x[i2]) + ...) / n — an
    explicit loop, one float32 add per row; a class without rows is a zero row; a label outside [0, C) is skipped and sets error = 1"""
    x = np.asarray(x, dtype=np.float32)
    N, D = x.shape
    acc = [None] * num_classes
    count = np.zeros(num_classes, dtype=np.int32)
    error = 0
    for i in range(N):
        c = int(labels[i])
        if not 0 <= c < num_classes:
            error = 1
            continue
        acc[c] = x[i].copy() if acc[c] is None else (acc[c] + x[i]).astype(np.float32)
        count[c] += 1
    mean = np.zeros((num_classes, D), dtype=np.float32)
    for c in range(num_classes):
        if acc[c] is not None:
            mean[c] = acc[c] / np.float32(count[c])
    return mean, count, error


def class_embeddings(dna_feature: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """float32 [D, C] (squeezed): the class means of np.unique(labels) in that order, as the reference's table"""
    all_label, dense = np.unique(np.asarray(labels).reshape(-1), return_inverse=True)
    return class_mean(dna_feature, dense, len(all_label))[0].T.squeeze()


def savetxt_text(table: np.ndarray) -> str:
    buf = io.StringIO()
    np.savetxt(buf, table, delimiter=",")
    return buf.getvalue()


def logits_topk(logits: torch.Tensor, k: int):
    """(values, indices) of torch.sort(descending=True, stable=True) cut to k columns, on the CPU"""
    v, i = torch.sort(logits.detach().cpu().float(), dim=1, descending=True, stable=True)
    return v[:, :k].contiguous(), i[:, :k].contiguous()


def topk_accuracies(idx: np.ndarray, target: np.ndarray, k_values=(1, 3, 5)) -> dict:
    """fine_tuning_epoch.py's accuracy of a prediction matrix"""
    return {f"top{k}_accuracy": np.mean(np.any(idx[:, :k] == target[:, None], axis=1)) for k in k_values}
