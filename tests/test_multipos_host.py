"""What the multi-positive InfoNCE feature promises without a device: `drivers --positives` parsing, the ValueError paths, the key
hashes against their numpy uint64 restatement, and the presence of the two entry points in the header and the ctypes table."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multipos_ref  # noqa: E402
from incremental_multimodal_medical_learning_ii_amd import _lib, contrastive as C, drivers, functional as Fh  # noqa: E402


def test_drivers_positives_argument():
    ap = drivers.make_parser()
    assert ap.parse_args(["class-inc", "--joint"]).positives == "pair"
    for v in ("pair", "labels", "text"):
        assert ap.parse_args(["class-inc", "--joint", "--positives", v]).positives == v
    with pytest.raises(SystemExit):
        ap.parse_args(["class-inc", "--joint", "--positives", "soft"])
    with pytest.raises(SystemExit, match="--joint"):                                 # rejected the way --text-dropout is
        drivers.main(["class-inc", "--positives", "labels"])


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cxrk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("cxrk_multipos_row_stats", 13), ("cxrk_multipos_grad_inplace", 10)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1])
        assert sum(a.startswith("const long long*") for a in args) == 2 and args[-1] == "hipStream_t stream"
        assert not any(re.search(r"\bws\b", a) for a in args)                        # no workspace: scratch is a caller's output
    assert "keys_row[i]==keys_col[j]" in hdr.replace(" ", "")                        # the formula is in the comment


def test_row_keys_match_the_numpy_restatement_and_ignore_padding():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-(1 << 40), 1 << 40, (9, 11), generator=g)
    x[0] = torch.tensor([0, -1, (1 << 63) - 1, -(1 << 63), 1, 2, 3, 4, 5, 6, 7])
    m = (torch.rand(9, 11, generator=g) > 0.3).long()
    m[1] = 0                                                                          # an empty row: key 0
    k = C.row_keys(x, m)
    assert k.dtype == torch.int64 and k.shape == (9,) and int(k[1]) == 0
    assert np.array_equal(k.numpy(), multipos_ref.row_keys_numpy(x.numpy(), m.numpy()))
    assert np.array_equal(C.row_keys(x).numpy(), multipos_ref.row_keys_numpy(x.numpy()))
    assert torch.equal(C.row_keys(x, m.bool()), k)
    # masked-out positions: neither their content nor their number matters
    x2 = x.clone()
    x2[m == 0] = 12345
    assert torch.equal(C.row_keys(x2, m), k)
    ids = torch.tensor([[5, 9, 9, 2, 0, 0], [5, 9, 9, 2, 7, 7], [5, 9, 2, 9, 0, 0], [5, 9, 9, 0, 0, 0]])
    msk = torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0]])
    kt = C.keys_from_tokens(ids, msk)
    longer = C.keys_from_tokens(torch.cat([ids, torch.full((4, 5), 3)], 1), torch.cat([msk, torch.zeros(4, 5, dtype=torch.long)], 1))
    assert torch.equal(kt, longer)                                                    # the same sentences, more trailing padding
    assert kt[0] == kt[1] and len({int(v) for v in kt}) == 3                          # order and length matter, padding does not


def test_keys_from_labels():
    lab = torch.tensor([[0., 1, 0, 0, 1], [0, 1, 0, 0, 1], [1, 1, 0, 0, 1], [0, 0, 0, 0, 0], [0, 1, 0, 1, 0]])
    k = C.keys_from_labels(lab)
    assert k[0] == k[1] and len({int(v) for v in k}) == 4
    assert torch.equal(k, C.keys_from_labels(lab.long())) and torch.equal(k, C.keys_from_labels(lab.double()))
    assert torch.equal(C.keys_from_labels(lab.bool()), k)
    assert np.array_equal(k.numpy(), multipos_ref.row_keys_numpy(lab.long().numpy()))
    for bad in (torch.tensor([[0.5, 1.0]]), torch.tensor([[float("nan"), 1.0]]), torch.tensor([[float("inf"), 1.0]])):
        with pytest.raises(ValueError, match="integral"):
            C.keys_from_labels(bad)
    with pytest.raises(ValueError):
        C.keys_from_labels(torch.zeros(5))
    with pytest.raises(ValueError):
        C.row_keys(torch.zeros(2, 3))                                                 # floats are not hashed


def test_infonce_keys_are_validated_before_anything_runs(monkeypatch):
    class NoKernels:
        def __getattr__(self, name):
            raise AssertionError(f"kernel wrapper {name} was reached before the keys were validated")
    monkeypatch.setattr(Fh, "K", NoKernels())
    img, txt = torch.zeros(8, 16), torch.zeros(8, 16)
    for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros(8), torch.zeros(7, dtype=torch.int64), torch.zeros(8, 1, dtype=torch.int64),
                torch.zeros(8, dtype=torch.int64, device="meta"), [0] * 8):
        with pytest.raises(ValueError, match="keys"):
            Fh.infonce_loss(img, txt, 0.07, None, keys=bad)


def test_trainer_positives_argument_and_key_selection():
    with pytest.raises(ValueError, match="positives"):
        C.JointContrastiveTrainer(None, None, positives="soft")
    ids = torch.tensor([[5, 9, 2, 0], [5, 9, 2, 0], [5, 8, 2, 1]])
    msk = torch.tensor([[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 1]])
    lab = torch.tensor([[1., 0], [0, 1], [0, 1]])
    mine = torch.tensor([4, 5, 6])

    def tr(positives):
        t = object.__new__(C.JointContrastiveTrainer)
        t.positives = positives
        return t
    assert tr(None).pair_keys(ids, msk) is None and tr(None).pair_keys(ids, msk, labels=lab) is None
    assert tr(None).pair_keys(ids, msk, keys=mine) is mine
    assert torch.equal(tr("text").pair_keys(ids, msk, labels=lab), C.keys_from_tokens(ids, msk))
    assert torch.equal(tr("labels").pair_keys(ids, msk, labels=lab), C.keys_from_labels(lab))
    assert tr("labels").pair_keys(ids, msk, labels=lab, keys=mine) is mine           # explicit keys win
    with pytest.raises(ValueError, match="labels"):
        tr("labels").pair_keys(ids, msk)
