"""Episodic memory of earlier tasks for the memory-based continual-learning methods: a fixed number of rows per
task, chosen by reservoir sampling from the task's stream of batches, kept on the batches' device in their own dtypes.

Every random choice is made on the host from a `torch.Generator` seeded by (seed, task index) or (seed, step): the same stream gives
the same memory, and the same step the same sample, on every data-parallel rank and in every run; nothing depends on a device value.
`JointContrastiveTrainer` draws A-GEM's reference batch from it; the rows come back as an ordinary batch, so replaying them beside
the training batch (experience replay) needs nothing more from this class."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

_MASK63 = (1 << 63) - 1


def _generator(seed: int, stream: int, index: int) -> torch.Generator:
    """a CPU generator keyed by (seed, stream, index): `stream` separates the draws of `add_task` (0) from those of `sample` (1)"""
    key = ((int(seed) * 0x9E3779B97F4A7C15) ^ ((2 * int(index) + int(stream) + 1) * 0xD1B54A32D192ED03)) & _MASK63
    return torch.Generator().manual_seed(key)


def _pad_tokens(t: torch.Tensor, width: int) -> torch.Tensor:
    """[rows, L] -> [rows, width], zeros on the right (id 0 under mask 0: padding, as the tokenizer writes it)"""
    if t.shape[1] == width:
        return t
    out = t.new_zeros((t.shape[0], width))
    out[:, :t.shape[1]] = t
    return out


class EpisodicMemory:
    FIELDS = ("images", "input_ids", "attention_mask", "extra")

    def __init__(self, rows_per_task: int, seed: int = 0):
        if isinstance(rows_per_task, bool) or not isinstance(rows_per_task, int) or rows_per_task < 1:
            raise ValueError(f"EpisodicMemory: rows_per_task must be an integer >= 1, got {rows_per_task!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"EpisodicMemory: seed must be an integer, got {seed!r}")
        self.rows_per_task, self.seed = rows_per_task, seed
        self.tasks: List[dict] = []          # one block per task: field -> tensor [rows, ...]
        self.width = 0                       # token width of every block

    def __len__(self) -> int:
        return sum(int(t["images"].shape[0]) for t in self.tasks)

    def _widen(self, width: int) -> None:
        if width > self.width:
            for t in self.tasks:
                t["input_ids"], t["attention_mask"] = _pad_tokens(t["input_ids"], width), _pad_tokens(t["attention_mask"], width)
            self.width = width

    @torch.no_grad()
    def add_task(self, batches) -> int:
        """Reservoir-sample (Algorithm R) `rows_per_task` rows from the stream of batches `(images, input_ids, attention_mask[, labels
        | keys])` into a new block -> the number of rows stored (the stream's length when it is shorter).  Row i of the stream
        (counted from 0) takes slot i while the block fills, and afterwards replaces slot j, drawn uniformly from 0..i, when
        j < rows_per_task.  Token rows narrower than the memory are right-padded with 0 in ids and mask; wider ones widen it."""
        R = self.rows_per_task
        gen = _generator(self.seed, 0, len(self.tasks))
        block: Optional[dict] = None
        seen = 0
        for batch in batches:
            if len(batch) not in (3, 4):
                raise ValueError(f"EpisodicMemory.add_task: a batch is (images, input_ids, attention_mask[, labels | keys]); got "
                                 f"{len(batch)} tensors")
            rows = int(batch[0].shape[0])
            if any(int(t.shape[0]) != rows for t in batch) or batch[1].dim() != 2 or batch[1].shape != batch[2].shape:
                raise ValueError("EpisodicMemory.add_task: the tensors of a batch must have the same number of rows, and the tokens "
                                 "and their mask the same [rows, L] shape")
            if rows == 0:
                continue
            self._widen(int(batch[1].shape[1]))
            fields = dict(zip(self.FIELDS, batch))
            for k in ("input_ids", "attention_mask"):
                fields[k] = _pad_tokens(fields[k], self.width)
            if block is None:
                if self.tasks:
                    first = self.tasks[0]
                    if set(first) != set(fields) or any(first[k].shape[1:] != v.shape[1:] or first[k].dtype != v.dtype
                                                        for k, v in fields.items()):
                        raise ValueError("EpisodicMemory.add_task: the rows of this task differ from the stored ones in their fields, "
                                         "shapes or dtypes")
                block = {k: v.new_empty((R,) + tuple(v.shape[1:])) for k, v in fields.items()}
            else:
                if set(block) != set(fields) or any(block[k].shape[1:] != v.shape[1:] and k not in ("input_ids", "attention_mask")
                                                    for k, v in fields.items()):
                    raise ValueError("EpisodicMemory.add_task: the batches of one task must agree in their fields and row shapes")
                for k in ("input_ids", "attention_mask"):
                    block[k] = _pad_tokens(block[k], self.width)
            # the draws of this batch's rows on the host, in stream order; a later row wins a slot taken twice
            idx = torch.arange(seen, seen + rows, dtype=torch.int64)
            draw = (torch.rand(rows, generator=gen, dtype=torch.float64) * (idx + 1).double()).long().clamp_(max=idx)
            slot = torch.where(idx < R, idx, draw)
            take = {}
            for r, s in enumerate(slot.tolist()):
                if s < R:
                    take[s] = r
            if take:
                dev = fields["images"].device
                both = torch.tensor([list(take.keys()), list(take.values())], dtype=torch.int64).to(dev)   # one index copy
                for k, v in fields.items():
                    block[k].index_copy_(0, both[0], v.index_select(0, both[1]).to(block[k].dtype))
            seen += rows
        if block is None:
            raise ValueError("EpisodicMemory.add_task: the stream of batches held no row")
        kept = min(seen, R)
        self.tasks.append({k: (v if kept == R else v[:kept].clone()) for k, v in block.items()})
        return kept

    @torch.no_grad()
    def sample(self, n: int, step: int) -> Tuple[torch.Tensor, ...]:
        """`n` distinct rows drawn uniformly over everything stored -> (images, input_ids, attention_mask[, labels | keys]).  The
        draw is the head of a host `randperm` seeded by (seed, step); the rows come back grouped by task, in the order drawn."""
        total = len(self)
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= total:
            raise ValueError(f"EpisodicMemory.sample: n must be an integer in [1, {total}] (the rows stored), got {n!r}")
        perm = torch.randperm(total, generator=_generator(self.seed, 1, step))[:n]
        local, counts, off = [], [], 0
        for t in self.tasks:
            rows = int(t["images"].shape[0])
            mine = perm[(perm >= off) & (perm < off + rows)] - off
            local.append(mine)
            counts.append(int(mine.numel()))
            off += rows
        index = torch.cat(local).to(self.tasks[0]["images"].device)                                          # one index copy
        parts, pos = [], 0
        for t, c in zip(self.tasks, counts):
            if c:
                parts.append({k: v.index_select(0, index[pos:pos + c]) for k, v in t.items()})
                pos += c
        keys = [k for k in self.FIELDS if k in parts[0]]
        return tuple(parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts]) for k in keys)

    def state_dict(self) -> dict:
        """tensors, lists and plain numbers only (loadable with weights_only=True)"""
        return {"rows_per_task": int(self.rows_per_task), "seed": int(self.seed), "width": int(self.width),
                "tasks": [{k: v.detach().cpu() for k, v in t.items()} for t in self.tasks]}

    @torch.no_grad()
    def load_state_dict(self, sd: dict, device=None) -> None:
        """strict: exactly the keys of `state_dict()`, written with this object's `rows_per_task` and `seed`; every block with the
        same fields, at most `rows_per_task` rows and token rows of the stated width.  The rows go to `device` (default: the host)."""
        want = {"rows_per_task", "seed", "width", "tasks"}
        if not isinstance(sd, dict) or set(sd) != want:
            raise ValueError(f"EpisodicMemory.load_state_dict: expected the keys {sorted(want)}, got "
                             f"{sorted(sd) if isinstance(sd, dict) else type(sd).__name__}")
        if int(sd["rows_per_task"]) != self.rows_per_task or int(sd["seed"]) != self.seed:
            raise ValueError(f"EpisodicMemory.load_state_dict: the state was written with rows_per_task={sd['rows_per_task']!r}, "
                             f"seed={sd['seed']!r}; this memory has {self.rows_per_task}, {self.seed}")
        tasks, width = sd["tasks"], int(sd["width"])
        if not isinstance(tasks, (list, tuple)):
            raise ValueError(f"EpisodicMemory.load_state_dict: 'tasks' must be a list, got {type(tasks).__name__}")
        for i, t in enumerate(tasks):
            need = set(self.FIELDS[:3])
            if not isinstance(t, dict) or not need <= set(t) or set(t) - set(self.FIELDS) or set(t) != set(tasks[0]):
                raise ValueError(f"EpisodicMemory.load_state_dict: task {i} must hold {sorted(need)} (and 'extra' in all tasks or none)")
            if not all(isinstance(v, torch.Tensor) for v in t.values()):
                raise ValueError(f"EpisodicMemory.load_state_dict: task {i} holds something other than tensors")
            rows = int(t["images"].shape[0])
            if not 1 <= rows <= self.rows_per_task or any(int(v.shape[0]) != rows for v in t.values()):
                raise ValueError(f"EpisodicMemory.load_state_dict: task {i} must hold between 1 and {self.rows_per_task} rows, the "
                                 f"same number in every field")
            if tuple(t["input_ids"].shape) != (rows, width) or tuple(t["attention_mask"].shape) != (rows, width):
                raise ValueError(f"EpisodicMemory.load_state_dict: the token rows of task {i} must be [{rows}, {width}]")
            if any(t[k].shape[1:] != tasks[0][k].shape[1:] or t[k].dtype != tasks[0][k].dtype for k in t):
                raise ValueError(f"EpisodicMemory.load_state_dict: task {i} differs from task 0 in a row shape or dtype")
        if not tasks and width != 0:
            raise ValueError("EpisodicMemory.load_state_dict: an empty memory has width 0")
        self.tasks = [{k: (v.to(device) if device is not None else v).clone() for k, v in t.items()} for t in tasks]
        self.width = width
