"""Packing plan of a padded batch: which rows of ``[B, L]`` are real tokens.

The toolkit's collators pad every batch to a fixed length (``padding='max_length'``), so the
attention mask of a batch is a prefix of ones per row.  ``plan_packing`` recognises exactly that
shape and describes the packed layout the padding-free inference path computes on
(``HipBertEncoder.forward_packed``): the ``T = sum(len_b)`` real tokens as one ``[T, H]`` matrix,
sequence ``b`` at rows ``cu_seqlens[b] .. cu_seqlens[b + 1] - 1``.  Any other mask gives ``None``
and the caller keeps the padded path.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

# The smallest padding share 1 - T / (B L) at which plan_packing packs.  Measured on BERT-base
# (tools/packed_encode_ab.py, profiles/packed01/packed_encode_ab.json): packed / padded time is
# 0.80 at a padding share of 0.31 and 1.03 with no padding at all and the plan forced (the plan's
# device-to-host copy and the unpack copy buy nothing there), so the two lines cross near a share
# of 0.04; 0.10 leaves that margin.  DESIGN.md §4 "Padding-free inference".
hip_packed_min_saving = 0.10

# The same threshold for the packed TRAINING tower (DRModel.hip_packed_train; model/train_tower.py).
# Measured on BERT-base, forward + backward of one tower with dropout (tools/packed_train_ab.py,
# profiles/packed_train01/packed_train_ab.json): packed / padded time is 0.60 at a padding share of
# 0.60, 0.76 at 0.37, 0.86 at 0.31 (256 x 160, the smallest GEMMs) and 1.05 with no padding at all and
# the plan forced (the plan's device-to-host copy drains the launch queue once per step).  The line
# from the control through the least favourable shape (256 x 160) crosses 1.0 at a share of 0.08, the
# other two near 0.06; with the margin of 0.06 that the inference threshold got over its crossing,
# rounded up: 0.15.  DESIGN.md §5 "Padding-free training".
hip_packed_train_min_saving = 0.15

# Attention length classes: ceil(len / 32) = 1 .. 5 run the kernels that hold the sequence's key
# blocks in registers, class 0 (len > 160) the streamed form.
_CLASS_MAX_BLOCKS = 5


@dataclass
class PackingPlan:
    lens: List[int]                   # host: tokens per sequence
    cu_seqlens: torch.Tensor          # device int32 [B + 1]
    T: int
    max_len: int
    B: int
    L: int
    # attention launches, one per length class present in the batch: (seq_ids device int32 or None
    # for "every sequence", n_seqs, max_len of the class); built on first use
    _classes: Optional[List[Tuple[Optional[torch.Tensor], int, int]]] = field(default=None, repr=False)
    _halves: Optional[list] = field(default=None, repr=False)

    def halves(self):
        """((first sequence, plan) x 2) splitting the batch at the sequence boundary nearest T / 2
        (B >= 2): two independent packed batches for the two-stream forward."""
        if self._halves is None:
            acc, cut, cut_row = 0, 1, self.lens[0]
            for b in range(1, self.B):
                acc += self.lens[b - 1]
                if abs(acc - self.T / 2) < abs(cut_row - self.T / 2):
                    cut, cut_row = b, acc
            cu = self.cu_seqlens     # the halves' tables from this one, on its device: no copy from the host
            first, second = self.lens[:cut], self.lens[cut:]
            self._halves = [
                (0, PackingPlan(first, cu[:cut + 1], cut_row, max(first), cut, self.L)),
                (cut, PackingPlan(second, cu[cut:] - cu[cut:cut + 1], self.T - cut_row, max(second), self.B - cut,
                                  self.L))]
        return self._halves

    def classes(self):
        """One (seq_ids, n_seqs, max_len) per attention launch: the sequences grouped by
        ceil(len / 32) up to 5 blocks, longer ones together.  A batch of one class needs no list."""
        if self._classes is None:
            groups = {}
            for b, n in enumerate(self.lens):
                nb = (n + 31) // 32
                groups.setdefault(nb if nb <= _CLASS_MAX_BLOCKS else 0, []).append(b)
            if len(groups) == 1:
                self._classes = [(None, self.B, self.max_len)]
            else:
                order = sorted(groups, key=lambda c: (c == 0, c), reverse=True)   # longest first
                flat = torch.tensor([b for c in order for b in groups[c]], dtype=torch.int32)
                flat = flat.to(self.cu_seqlens.device)
                out, at = [], 0
                for c in order:
                    ids = groups[c]
                    out.append((flat[at:at + len(ids)], len(ids), max(self.lens[b] for b in ids)))
                    at += len(ids)
                self._classes = out
        return self._classes

    def launches(self, per_class: bool):
        """The (seq_ids pointer or None, n_seqs, max_len) of each varlen attention launch over the batch,
        forward or backward: one per length class (``classes()``), or one for the whole batch.  Callers
        build it once per pass, outside their layer loop."""
        launches = self.classes() if per_class else [(None, self.B, self.max_len)]
        return [(s.data_ptr() if s is not None else None, n, ml) for s, n, ml in launches]


def _plan_from_lens(lens: List[int], L: int, device, min_saving: float, force: bool) -> Optional[PackingPlan]:
    B = len(lens)
    T = sum(lens)
    if not force and (T == B * L or 1.0 - T / float(B * L) < min_saving):
        return None
    cu = [0] * (B + 1)
    for b, n in enumerate(lens):
        cu[b + 1] = cu[b] + n
    cu_t = torch.tensor(cu, dtype=torch.int32)
    if device is not None and torch.device(device).type != "cpu":
        cu_t = cu_t.to(device)
    return PackingPlan(lens=lens, cu_seqlens=cu_t, T=T, max_len=max(lens), B=B, L=L)


def plan_packing(attention_mask: Optional[torch.Tensor], L: int, device=None,
                 min_saving: Optional[float] = None, force: bool = False) -> Optional[PackingPlan]:
    """The packing plan of a ``[B, L]`` attention mask, or ``None`` for "use the padded path":
    no mask, a row that is not a non-empty prefix of ones (holes, left padding, an all-zero row), no
    padding at all (``T == B L``), or a padding share below ``min_saving`` (default
    ``hip_packed_min_saving``).  ``force`` keeps a full batch packed (measurements).

    A mask on the GPU costs exactly one device-to-host copy, which carries the lengths and the
    prefix verdict together; a CPU mask is planned on the CPU with no synchronisation.
    ``cu_seqlens`` lands on ``device`` (default: the mask's device)."""
    if attention_mask is None:
        return None
    m = attention_mask
    if m.dim() != 2 or m.shape[1] != L or m.shape[0] == 0 or L == 0:
        return None
    B = m.shape[0]
    nz = m != 0
    lens = nz.sum(1, dtype=torch.int64)                                   # [B]
    # a prefix of ones is the pattern "position < len" itself
    prefix = (nz == (torch.arange(L, device=m.device)[None, :] < lens[:, None])).all(1) & (lens > 0)
    verdict = torch.cat([lens, prefix.all().to(torch.int64).reshape(1)])   # one tensor, one copy
    host = verdict.tolist() if m.device.type == "cpu" else verdict.cpu().tolist()
    if not host[B]:
        return None
    if min_saving is None:
        min_saving = hip_packed_min_saving
    return _plan_from_lens([int(x) for x in host[:B]], L, device if device is not None else m.device,
                           min_saving, force)
