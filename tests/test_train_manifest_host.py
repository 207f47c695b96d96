"""Manifest datasets without h5py (cbas_amd/datasets.py) on the host: sample order and window values against what the
reference's LazyStandardDataset / LazyBalancedDataset / Project.convert_instances produced
(tests/golden/train_manifest_order.npz, recorded by tests/golden/make_goldens_manifest.py), resolve() against
__getitem__, the refusals and dropped samples, and the recognition of manifest datasets by their attribute names."""
import os

import numpy as np
import pytest
import torch

from cbas_amd import h5io, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "train_manifest_order.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def project(fx, tmp_path_factory):
    """The fixture's synthetic project, written again from its recorded settings."""
    root = str(tmp_path_factory.mktemp("manifest_project"))
    behaviors = [str(b) for b in fx["behaviors"]]
    paths, labels = synth.cls_project(root, fx["sizes"].tolist(), int(fx["dim"]), len(behaviors), int(fx["seed"]),
                                      skip_classes=tuple(fx["skip_classes"].tolist()))
    paths.append(os.path.join(root, "clip4_cls.h5"))                    # the fixture's missing file
    return paths, behaviors


def fixture_manifest(fx, paths):
    return [(paths[f], int(c), int(l)) for f, c, l in zip(fx["manifest/file"], fx["manifest/centre"], fx["manifest/label"])]


def recording(cls):
    """The dataset class with resolve() logging the manifest indices it hands to __getitem__."""
    class Recording(cls):
        def resolve(self, idx):
            m = super().resolve(idx)
            self.taken.append(m)
            return m
    return Recording


def test_make_manifest_reproduces_convert_instances(fx, project):
    from cbas_amd.datasets import make_manifest
    paths, behaviors = project
    inst = [(paths[f], int(a), int(b), str(lab)) for f, a, b, lab in zip(fx["inst/file"], fx["inst/start"], fx["inst/end"], fx["inst/label"])]
    got = make_manifest(inst, int(fx["seq_len"]), behaviors)
    assert got == fixture_manifest(fx, paths)
    # the cases the instance list was built to hold: clipped at both ends, and nothing from files 3 (short) and 4 (missing)
    files = np.array([paths.index(m[0]) for m in got])
    half = int(fx["seq_len"]) // 2
    assert set(files.tolist()) == {0, 1, 2}
    for f in range(3):
        centres = np.array([m[1] for m in got if m[0] == paths[f]])
        assert centres.min() == half and centres.max() == int(fx["sizes"][f]) - half - 1


@pytest.mark.parametrize("tag", ["standard", "balanced"])
def test_sample_order_and_windows_match_the_reference(fx, project, tag):
    from cbas_amd import datasets as D
    paths, behaviors = project
    T, stride = int(fx["seq_len"]), int(fx["stride"])
    manifest = fixture_manifest(fx, paths)
    if tag == "standard":
        ds = recording(D.LazyStandardDataset)(manifest, T)
    else:
        ds = recording(D.LazyBalancedDataset)(manifest, T, behaviors)
        assert ds.available_behaviors == [str(b) for b in fx["balanced/available"]] and ds.total_sequences == len(manifest)
        assert all(len(ds.buckets[b]) == int((fx["manifest/label"] == i).sum()) for i, b in enumerate(behaviors))
    assert len(ds) == int(fx[f"{tag}/len"])
    assert ds.manifest is manifest and ds.seq_len == T
    g = torch.Generator()
    g.manual_seed(int(fx["loader_seed"]))
    loader = torch.utils.data.DataLoader(ds, int(fx["batch"]), shuffle=True, num_workers=0, generator=g)
    for p in range(int(fx["passes"])):
        ds.taken = []
        labels, values = [], []
        for x, y in loader:
            assert x.dtype == torch.float32 and y.dtype == torch.int64 and tuple(x.shape[1:]) == (T, int(fx["dim"]))
            labels.append(y.numpy())
            values.append(x.numpy().reshape(-1))
        taken = [manifest[m] for m in ds.taken]
        assert np.array_equal([paths.index(t[0]) for t in taken], fx[f"{tag}/pass{p}/file"]), p
        assert np.array_equal([t[1] for t in taken], fx[f"{tag}/pass{p}/centre"]), p
        assert np.array_equal(np.concatenate(labels), fx[f"{tag}/pass{p}/label"]), p
        got = np.concatenate(values)[::stride]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), fx[f"{tag}/pass{p}/values"].view(np.uint32)), p
    if tag == "balanced":
        assert ds.counter == int(fx["balanced/counter"]) == int(fx["passes"]) * len(ds)
    D.close_readers()


def test_resolve_and_getitem_agree(fx, project):
    """The same index sequence through resolve() and through __getitem__: the same samples, the counter advanced equally;
    the helpers for foreign objects (resolve_index / balanced_len) give the same again on a plain stand-in."""
    from cbas_amd import datasets as D
    paths, behaviors = project
    T = int(fx["seq_len"])
    manifest = fixture_manifest(fx, paths)
    idx = torch.randperm(896, generator=torch.Generator().manual_seed(3)).tolist() + [5, 5, 0, 895]

    class Foreign:                       # only the reference's attribute names, no resolve()
        def __len__(self):
            return 896
    for make in (lambda: D.LazyStandardDataset(manifest, T), lambda: D.LazyBalancedDataset(manifest, T, behaviors)):
        a, b, c = make(), make(), make()
        f = Foreign()
        f.__dict__.update(c.__dict__)
        balanced = hasattr(a, "counter")
        use = idx if balanced else [i for i in idx if i < len(manifest)]
        for i in use:
            m = a.resolve(i)
            x, y = b[i]
            assert m == D.resolve_index(f, i)
            path, centre, label = manifest[m]
            assert int(y) == label
            with h5io.ClsReader(path) as r:
                want = r.read(centre - T // 2, centre + T // 2 + 1)
            assert want.dtype == np.float16 and np.array_equal(x.numpy(), want.astype(np.float32))
        if balanced:
            assert a.counter == b.counter == f.counter == len(use)
            assert D.balanced_len(f) == len(a) == 896
    D.close_readers()


def test_refusals_and_dropped_samples(tmp_path):
    from cbas_amd import datasets as D
    good, other, bad = str(tmp_path / "a_cls.h5"), str(tmp_path / "b_cls.h5"), str(tmp_path / "c_cls.h5")
    rows = synth.cls_walk(1, 50, 64)
    with h5io.ClsWriter(good, 64) as w:
        w.append(rows)
    with h5io.ClsWriter(other, 96) as w:
        w.append(synth.cls_walk(2, 40, 96))
    with open(bad, "wb") as f:
        f.write(b"this is not an HDF5 file" * 40)
    missing = str(tmp_path / "nowhere_cls.h5")
    manifest = [(good, 20, 1), (bad, 20, 0), (missing, 20, 0), (good, 3, 1), (good, 46, 0), (good, 4, 1), (good, 45, 0)]
    for ds in (recording(D.LazyStandardDataset)(manifest, 9), recording(D.LazyBalancedDataset)(manifest, 9, ["x", "y"])):
        ds.taken, got = [], {}
        for i in range(24):                         # i // 2: the balanced class alternates its two buckets, so each sees 0..11
            x, y = ds[(i // 2) % len(manifest)]
            got[ds.taken[-1]] = (x, int(y))
        assert set(got) == set(range(len(manifest)))
        for m, (x, y) in got.items():
            assert x.dtype == torch.float32 and x.shape[0] == 9
            if m in (1, 2, 3, 4):                   # unreadable, missing, reaching before row 0, reaching past the last row
                assert y == -1 and not x.any(), m
            else:                                   # 4 and 45 are the first and last centres whose window is inside the file
                c = manifest[m][1]
                assert y == manifest[m][2] and np.array_equal(x.numpy(), rows[c - 4:c + 5].astype(np.float32)), m
    D.close_readers()
    # an even seq_len makes the window seq_len + 1 rows: refused, and said so
    for make in (lambda: D.LazyStandardDataset(manifest, 8), lambda: D.LazyBalancedDataset(manifest, 8, ["x", "y"]),
                 lambda: D.make_manifest([(good, 0, 10, "x")], 30, ["x"])):
        with pytest.raises(ValueError, match="odd"):
            make()
    # store layout: unreadable files get no rows and their entries drop; a second row width is refused by name
    plan = D.plan_store([manifest], 64)
    assert plan.files == {good: (0, 50)} and set(plan.unreadable) == {bad, missing} and plan.nbytes == 50 * 64 * 2
    first, label = D.manifest_windows(manifest, 9, plan.files)
    assert first.tolist() == [16, -1, -1, -1, -1, 0, 41] and label.tolist() == [1, -1, -1, -1, -1, 1, 0]
    with pytest.raises(ValueError, match="b_cls.h5"):
        D.plan_store([manifest, [(other, 20, 0)]], 64)
    with pytest.raises(ValueError, match="a_cls.h5"):
        D.plan_store([manifest], 768)


def test_manifest_datasets_are_recognised_by_attribute_names():
    from cbas_amd import datasets as D

    class Std:                           # the reference's LazyStandardDataset, as far as its attributes go
        def __init__(self):
            self.manifest, self.seq_len, self.half_seqlen = [("f", 20, 0), ("f", 21, 1), ("f", 22, 1)], 31, 15

        def __len__(self):
            return len(self.manifest)

        def __getitem__(self, i):
            raise AssertionError("needs h5py: must never be called")

    class Bal(Std):                      # ... and its LazyBalancedDataset
        def __init__(self):
            super().__init__()
            self.behaviors, self.num_behaviors = ["a", "b", "c"], 3
            self.buckets = {"a": [0], "b": [1, 2], "c": []}
            self.available_behaviors, self.num_available_behaviors = ["a", "b"], 2
            self.total_sequences, self.counter = 3, 0

        def __len__(self):
            return 4

    class Plain(torch.utils.data.Dataset):
        def __len__(self):
            return 3

        def __getitem__(self, i):
            return torch.zeros(31, 8), torch.tensor(0)

    assert D.manifest_kind(Std()) == "standard" and D.manifest_kind(Bal()) == "balanced"
    assert D.manifest_kind(Plain()) is None and D.manifest_kind(None) is None and D.manifest_kind([1, 2]) is None
    assert D.manifest_kind(D.LazyStandardDataset([], 31)) == "standard"
    assert D.manifest_kind(D.LazyBalancedDataset([], 31, ["a"])) == "balanced"
    s, b = Std(), Bal()
    assert [D.resolve_index(s, i) for i in (2, 0, 1)] == [2, 0, 1]
    # round-robin over the classes that have samples, bucket[idx % len(bucket)], the counter carried on the instance
    assert [D.resolve_index(b, i) for i in (3, 3, 2, 2, 0, 1)] == [0, 2, 0, 1, 0, 2] and b.counter == 6
    assert D.balanced_len(b) == 4
    # the decision train_lstm_model takes from it needs no GPU either: an ordinary dataset keeps the host loader
    from cbas_amd.train import plan_training_data
    plan, line = plan_training_data(Plain(), None, 31, 8, "cuda")
    assert plan is None and line.startswith("training data: host loader")
