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

# The threshold for a batch whose longest sequence is over 160 tokens (hip_packed_train_long).  Measured the same
# way (tools/packed_train_ab.py --long, profiles/packed_train_long01/packed_train_long_ab.json): packed / padded
# is 0.897 at a padding share of 0.311 (128 x 256), 0.895 at 0.281 (64 x 512) and 1.061 with no padding and
# the plan forced -- the plan's device-to-host copy costs 1.3 ms of a 26 ms step, a larger part than of the
# 41 ms steps above.  The lines from the control cross 1.0 at shares of 0.115 and 0.10; with the same margin
# of 0.06: 0.18.  DESIGN.md §5 "Padding-free training above 160 tokens".
hip_packed_train_long_min_saving = 0.18

# The whole-sequence attention kernels hold a sequence's key blocks in registers: ceil(len / 32) = 1 .. 5,
# kAbMaxSeq of csrc/drt_common.h.  Longer sequences run the streamed forms -- in inference one class of
# their own (class 0 of ``classes()``); in the packed training tower (``split()``) the streamed pair over
# 128-row tiles, its forward's launch classes by LDS image (260 B per padded key): up to 192 keys three
# work-groups share a CU's 160 KiB, up to 288 two, beyond that one.
_SHORT_MAX = 160
_CLASS_MAX_BLOCKS = _SHORT_MAX // 32
_TILE_ROWS = 128
_LONG_CLASS_MAX = (192, 288, 512)


def _short_class(n: int) -> int:
    return min((n + 31) // 32, _CLASS_MAX_BLOCKS + 1)


class _OnFirstUse(dict):
    """{key: build(key)}, each value built when it is first asked for."""

    def __init__(self, build):
        super().__init__()
        self._build = build

    def __missing__(self, key):
        self[key] = self._build(key)
        return self[key]


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
    _split: Optional[dict] = field(default=None, repr=False)

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

    def _group(self, ids, class_of):
        """{False: one launch over the sequences ``ids``, True: one per class ``class_of(len)``, longest
        first}, each launch (seq_ids, n_seqs, max_len) with seq_ids a slice of one device tensor, or None
        ("every sequence") where a single launch covers the whole batch.  A list is grouped, and its ids are
        copied to the device, when it is first asked for: the grouping is O(B) on the host and the copy
        waits for the stream, once per training step."""
        if not ids:
            return {False: [], True: []}

        def build(per_class):
            if not per_class and len(ids) == self.B:
                return [(None, self.B, self.max_len)]
            groups = {}
            for b in ids:
                groups.setdefault(class_of(self.lens[b]), []).append(b)
            parts = [groups[c] for c in sorted(groups, reverse=True)]
            launches = parts if per_class else [[b for part in parts for b in part]]
            if len(launches) == 1 and len(ids) == self.B:
                return [(None, self.B, self.max_len)]
            flat = torch.tensor([b for part in parts for b in part], dtype=torch.int32).to(self.cu_seqlens.device)
            ends = [sum(len(part) for part in launches[:i + 1]) for i in range(len(launches))]
            return [(flat[e - len(part):e], len(part), max(self.lens[b] for b in part)) for part, e in zip(launches, ends)]

        return _OnFirstUse(build)

    def classes(self):
        """One (seq_ids, n_seqs, max_len) per attention launch: the sequences grouped by
        ceil(len / 32) up to 5 blocks, longer ones together (class 0, first).  A batch of one class needs
        no list."""
        if self._classes is None:
            self._classes = self._group(list(range(self.B)), _short_class)[True]
        return self._classes

    def split(self):
        """The batch as the packed TRAINING tower differentiates it: a dict, built once, of
        ``short`` / ``long``: [(seq_ids, n_seqs, max_len)] per attention launch of the sequences of at
        most / over 160 tokens, keyed by ``per_class`` (False: one launch per part; True: the short ones
        by length class as ``classes()``, the long ones by the LDS image of the forward: up to
        ``_LONG_CLASS_MAX`` tokens each); ``tiles``: device int32 [n_tiles, 2] = (sequence, 128-row
        group) of every group of a long sequence that holds a token, a sequence's groups adjacent;
        ``n_tiles``.  With no sequence over 160 tokens the long part and the tile table are empty and the
        short part is ``launches(per_class)``."""
        if self._split is None:
            long_ = [b for b, n in enumerate(self.lens) if n > _SHORT_MAX] if self.max_len > _SHORT_MAX else []
            short = [b for b, n in enumerate(self.lens) if n <= _SHORT_MAX] if long_ else list(range(self.B))
            tiles = [(b, g) for b in long_ for g in range((self.lens[b] + _TILE_ROWS - 1) // _TILE_ROWS)]
            self._split = {
                "short": self._group(short, _short_class),
                "long": self._group(long_, lambda n: next(i for i, m in enumerate(_LONG_CLASS_MAX) if n <= m)),
                "tiles": torch.tensor(tiles, dtype=torch.int32, device=self.cu_seqlens.device).reshape(-1, 2),
                "n_tiles": len(tiles)}
        return self._split

    def launches(self, per_class: bool, part: Optional[str] = None):
        """The (seq_ids pointer or None, n_seqs, max_len) of each varlen attention launch over the batch,
        forward or backward: one per length class (``classes()``), or one for the whole batch.  ``part`` =
        "short" / "long": the launches of that part of ``split()`` instead."""
        launches = self.split()[part][bool(per_class)] if part else \
            self.classes() if per_class else [(None, self.B, self.max_len)]
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
