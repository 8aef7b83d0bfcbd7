"""The host code around the joint step that needs neither a device nor the library: `Trainer.joint_options` (the one table that maps
`joint_encoders` onto `JointContrastiveTrainer.__init__`), `Trainer.end_task`, `Trainer._joint_shard` and the `joint_encoders` dict
the drivers assemble."""
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from incremental_multimodal_medical_learning_ii_amd import Trainer as TR  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import contrastive as C, drivers  # noqa: E402

NOT_OFFERED = {"image_model", "text_model", "lr", "group", "train_mlm_head", "two_streams"}    # `Trainer` passes or withholds these
GROUPS = {"ewc_lambda": ("ewc_gamma", "ewc_fisher", "ewc_batches"), "distill_weight": ("distill_temperature",),
          "agem_memory": ("agem_batch", "agem_every", "agem_seed")}
VALUES = {"ewc_lambda": 10.0, "ewc_gamma": 0.5, "ewc_fisher": "identity", "ewc_batches": 2, "distill_weight": 1.0,
          "distill_temperature": 0.1, "agem_memory": 8, "agem_batch": 4, "agem_every": 2, "agem_seed": 3}


def test_an_unknown_key_is_refused_before_anything_is_built():
    """a misspelt key used to be ignored, and the run trained without the option; `object()` as the text engine proves that the
    refusal comes before the engine is touched"""
    with pytest.raises(ValueError, match="ewc_lamda") as e:
        TR.Trainer(True, [], [], "standard", 1e-3, "cpu", None, bert_encoder=object(),
                   joint_encoders={"image_model": object(), "ewc_lamda": 1.0})
    assert "'ewc_lambda'" in str(e.value) and "'contrastive_loss'" in str(e.value) and "'retrieval'" in str(e.value)   # the valid keys
    with pytest.raises(ValueError, match="loss"):
        TR.joint_options({"image_model": object(), "loss": "sigmoid"})          # the keyword's name is not the key
    with pytest.raises(ValueError, match="two_streams"):
        TR.joint_options({"image_model": object(), "two_streams": False})


def test_the_table_matches_the_signature():
    keywords = set(inspect.signature(C.JointContrastiveTrainer.__init__).parameters) - {"self"}
    reached = list(TR.JOINT_STEP_KEYS.values())
    assert sorted(reached) == sorted(keywords - NOT_OFFERED)                    # every offered keyword, from exactly one key
    assert set(TR.JOINT_RENAMED.values()) <= keywords and TR.JOINT_RENAMED == {"contrastive_loss": "loss"}
    assert not set(TR.JOINT_OWN_KEYS) & set(TR.JOINT_STEP_KEYS) and TR.JOINT_OWN_KEYS == ("image_model", "retrieval", "ewc_batches")
    assert {g[0]: g[1] for g in TR.JOINT_GROUPS} == GROUPS
    for master, members, _, _ in TR.JOINT_GROUPS:
        for k in (master,) + members:
            assert k in keywords or k in TR.JOINT_OWN_KEYS, k
    # what reaches the constructor: renamed, None and "augment": False as not given, the module's optimiser by default
    im = object()
    step, own = TR.joint_options({"image_model": im, "contrastive_loss": "sigmoid", "sigmoid_bias": None, "augment": False,
                                  "augment_seed": 5, "retrieval": (1, 2), "log_scale_bounds": (0.0, 1.0)})
    assert step == {"loss": "sigmoid", "temperature": 0.07, "optim": TR.OPTIM, "log_scale_bounds": (0.0, 1.0)}
    assert own == {"image_model": im, "retrieval": (1, 2), "ewc_batches": None}
    assert TR.joint_options((im, 0.2)) == ({"temperature": 0.2, "optim": TR.OPTIM}, {"image_model": im, "retrieval": None, "ewc_batches": None})
    assert TR.joint_options({"image_model": im, "optim": "adamw", "augment": True, "augment_seed": 5})[0] == {
        "temperature": 0.07, "optim": "adamw", "augment": True, "augment_seed": 5}


@pytest.mark.parametrize("master", sorted(GROUPS))
def test_group_checks(master):
    im = object()
    for member in GROUPS[master]:
        with pytest.raises(ValueError, match="without it") as e:
            TR.joint_options({"image_model": im, member: VALUES[member]})
        assert f"'{master}'" in str(e.value) and member in str(e.value)
        assert TR.joint_options({"image_model": im, member: None})[0].get(member) is None     # None: not given
    for key in (master,) + GROUPS[master]:
        for je in ({key: VALUES[key]}, {"image_model": None, key: VALUES[key]}):
            with pytest.raises(ValueError, match="joint mode") as e:
                TR.joint_options(je)
            assert key in str(e.value)
    step, own = TR.joint_options({"image_model": im, master: VALUES[master], **{m: VALUES[m] for m in GROUPS[master]}})
    assert {**step, **own}[master] == VALUES[master] and all({**step, **own}[m] == VALUES[m] for m in GROUPS[master])


class _Joint:
    def __init__(self, ewc, distill, memory):
        self.ewc, self.distill_weight, self.memory = (object() if ewc else None), (1.0 if distill else None), (object() if memory else None)


@pytest.mark.parametrize("ewc", [False, True])
@pytest.mark.parametrize("distill", [False, True])
@pytest.mark.parametrize("memory", [False, True])
def test_end_task_makes_the_configured_calls_in_order(ewc, distill, memory):
    calls, loader = [], object()
    t = TR.Trainer.__new__(TR.Trainer)
    t.consolidate = lambda ld: calls.append(("consolidate", ld))
    t.snapshot_teacher = lambda: calls.append(("snapshot_teacher",))
    t.remember = lambda ld: calls.append(("remember", ld))
    t._joint = _Joint(ewc, distill, memory)
    assert t.end_task(loader) is None
    assert calls == ([("consolidate", loader)] if ewc else []) + ([("snapshot_teacher",)] if distill else []) + (
        [("remember", loader)] if memory else [])
    del calls[:]
    t._joint = None                                                            # adapter mode
    t.end_task(loader)
    assert calls == []


BASE = {"temperature": 0.07, "positives": None, "learn_temperature": False, "contrastive_loss": "infonce", "sigmoid_bias": None,
        "micro_batch": None, "augment": None, "retrieval": None}


@pytest.mark.parametrize("argv, extra", [
    (["class-inc", "--joint"], {}),
    (["class-inc", "--joint", "--cl", "ewc"], {"ewc_lambda": 1e4}),
    (["data-inc", "--joint", "--cl", "ewc", "--ewc-lambda", "3e5", "--ewc-batches", "8", "--ewc-gamma", "0.9", "--ewc-fisher", "identity"],
     {"ewc_lambda": 3e5, "ewc_batches": 8, "ewc_gamma": 0.9, "ewc_fisher": "identity"}),
    (["class-inc", "--joint", "--cl", "lwf"], {"distill_weight": 1.0}),
    (["data-inc", "--joint", "--cl", "lwf", "--distill-weight", "0.5", "--distill-temperature", "0.2"],
     {"distill_weight": 0.5, "distill_temperature": 0.2}),
    (["data-inc", "--joint", "--cl", "lwf", "--distill-weight", "0"], {"distill_weight": 0.0}),
    (["class-inc", "--joint", "--cl", "agem"], {"agem_memory": 256}),
    (["data-inc", "--joint", "--cl", "agem", "--agem-memory", "64", "--agem-batch", "32", "--agem-every", "4"],
     {"agem_memory": 64, "agem_batch": 32, "agem_every": 4})])
def test_the_drivers_joint_encoders(argv, extra):
    """the whole dict `_setup` hands to `Trainer`, against a literal; and `Trainer` accepts every key of it"""
    im = object()
    je = drivers.joint_encoders_from_args(drivers.parse_args(argv), im)
    assert je == {"image_model": im, **BASE, **extra}
    step, own = TR.joint_options(je)
    assert step == {"temperature": 0.07, "learn_temperature": False, "loss": "infonce", "optim": TR.OPTIM,
                    **{k: v for k, v in extra.items() if k != "ewc_batches"}}
    assert own == {"image_model": im, "retrieval": None, "ewc_batches": extra.get("ewc_batches")}


def _bare_trainer(positives, world=1, rank=0):
    t = TR.Trainer.__new__(TR.Trainer)
    t._joint = C.JointContrastiveTrainer.__new__(C.JointContrastiveTrainer)
    t._joint.positives = positives
    t.device, t.world, t.rank = torch.device("cpu"), world, rank
    return t


def _loader_batch():
    g = torch.Generator().manual_seed(5)
    images = torch.rand(4, 3, 2, 2, generator=g)
    ids = torch.randint(0, 50, (4, 3), generator=g)
    ids[2] = ids[0]                                                             # rows 0 and 2: one report
    mask = torch.ones(4, 3, dtype=torch.int64)
    labels = (torch.rand(4, 5, generator=g) < 0.5).float()
    labels[3] = labels[1]                                                       # rows 1 and 3: one label vector
    return images, ids, mask, labels


@pytest.mark.parametrize("world, rank", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("positives", [None, "text", "labels"])
def test_joint_shard_rows_and_keys(positives, world, rank):
    batch = _loader_batch()
    rows = slice(0, 4) if world == 1 else slice(2 * rank, 2 * rank + 2)
    images, ids, mask, keys = _bare_trainer(positives, world, rank)._joint_shard(batch)
    assert torch.equal(images, batch[0][rows]) and torch.equal(ids, batch[1][rows]) and torch.equal(mask, batch[2][rows])
    want = {None: None, "text": C.keys_from_tokens(batch[1], batch[2]), "labels": C.keys_from_labels(batch[3])}[positives]
    if want is None:
        assert keys is None
    else:
        assert keys.dtype == torch.int64 and torch.equal(keys, want[rows])
        pair = (0, 2) if positives == "text" else (1, 3)
        assert want[pair[0]] == want[pair[1]] and len(set(want.tolist())) == 3     # the keys mean what they should
    # the three-tensor batch serves unless the labels are the positives
    if positives != "labels":
        short = _bare_trainer(positives, world, rank)._joint_shard(batch[:3])
        assert torch.equal(short[0], images) and (short[3] is None) == (keys is None)
    shards = list(_bare_trainer(positives, world, rank)._joint_shards([batch], "consolidate"))
    assert len(shards) == 1 and len(shards[0]) == (3 if positives is None else 4) and torch.equal(shards[0][1], ids)


def test_joint_shard_refusals():
    batch = _loader_batch()
    for who in ("joint-encoder training", "Trainer.remember"):
        with pytest.raises(ValueError, match=r"expects loaders that yield \(images, input_ids, attention_mask\[, labels\]\); got a batch of 2 tensors") as e:
            _bare_trainer(None)._joint_shard(batch[:2], who)
        assert str(e.value).startswith(who + " ")
        with pytest.raises(ValueError, match=r"needs the labels: the loader must yield \(images, input_ids, attention_mask, labels \[B, C\]\)") as e:
            _bare_trainer("labels")._joint_shard(batch[:3], who)
        assert str(e.value).startswith(who + " ")
    odd = tuple(t[:3] for t in batch)
    with pytest.raises(ValueError, match=r"retrieval evaluation shards the batch evenly: 3 rows over 2 ranks \(use drop_last\)"):
        _bare_trainer(None, 2, 1)._joint_shard(odd, "retrieval evaluation")
    assert _bare_trainer(None)._joint_shard(odd)[0].shape[0] == 3                  # a single process takes any number of rows
