"""Synapse multi-organ trees from disk into the HBM-resident slice pool (reference datasets/Synapse.py:60-99, get_synapse_loader :117-132,
get_ssl_synapse_loader :135-153).

Directory contract of the reference (the TransUNet preprocessing): ``<root>/train.txt`` names 2-D training slices stored as
``<root>/train_npz/<name>.npz`` (arrays ``image`` and ``label``, read with ``numpy.load``), ``<root>/test_vol.txt`` names volumes
``<root>/test_vol_h5/<name>.npy.h5`` (datasets ``image`` and ``label``, read with the dependency-free ``h5lite``; h5py is not part of the
image).  The reference's Synapse ``RandomGenerator`` is the ACDC one, so the training slices go into a ``DeviceSlicePool`` and are augmented
by ``DevicePoolLoader`` exactly like ACDC slices (``acdc.py``); every file is read once.  The labelled / unlabelled split is
``torch.utils.data.random_split``'s law: a permutation from torch's default generator, first ``int(len * label_num)`` indices labelled
(Synapse.py:145-147).  Labels run 0 .. 8 (eight organs).
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from .acdc import _read_list
from .h5lite import read_datasets

NUM_CLASSES = 9


class SynapseFiles:
    """Host-side view of a Synapse root: the file list of a split (Synapse.py:87-99) and arrays on demand."""

    def __init__(self, root: str, split: str = "train"):
        self.root, self.split = root, split
        if split == "train":
            self.sample_list = [f"{root}/train_npz/{c}.npz" for c in _read_list(root + "/train.txt")]
        else:
            self.sample_list = [f"{root}/test_vol_h5/{c}.npy.h5" for c in _read_list(root + "/test_vol.txt")]

    def __len__(self):
        return len(self.sample_list)

    def __getitem__(self, idx) -> Tuple[np.ndarray, np.ndarray]:
        if self.split == "train":
            with np.load(self.sample_list[idx]) as d:          # Synapse.py:75-76
                image, label = d["image"], d["label"]
        else:
            d = read_datasets(self.sample_list[idx], ("image", "label"))          # Synapse.py:78-79
            image, label = d["image"], d["label"]
        return np.array(image, dtype=np.float32), np.array(label, dtype=np.uint8)

    def label_to_img(self, label):          # Synapse.py:101-114 (a spread of hues, not the reference's exact colours)
        from .synthetic import palette_image
        return palette_image(label, NUM_CLASSES)


class _Volumes(torch.utils.data.Dataset):
    """bs=1 evaluation volumes (image [S,h,w] float32, label [S,h,w] uint8), read once."""

    def __init__(self, files: SynapseFiles):
        self.items = [files[i] for i in range(len(files))]
        self.label_to_img = files.label_to_img

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        img, lab = self.items[i]
        return torch.from_numpy(img), torch.from_numpy(lab)


def _pool(root: str, device):
    from .device_pool import DeviceSlicePool
    files = SynapseFiles(root, "train")
    return DeviceSlicePool([files[i] for i in range(len(files))], device), len(files)


def _test_loader(root: str):
    return torch.utils.data.DataLoader(_Volumes(SynapseFiles(root, "test")), batch_size=1, shuffle=False)


def get_synapse_loader(root: str, batch_size: int = 8, train_crop_size: Sequence[int] = (224, 224), device="cuda"):
    """(train_loader, test_loader) like the reference's get_synapse_loader (Synapse.py:117-132)."""
    from .device_pool import DevicePoolLoader
    pool, _ = _pool(root, device)
    return DevicePoolLoader(pool, batch_size, train_crop_size), _test_loader(root)


def get_ssl_synapse_loader(root: str, batch_size: int = 8, unlabel_batch_size: int = 24, train_crop_size: Sequence[int] = (224, 224),
                           label_num: float = 0.2, device="cuda"):
    """(label_loader, unlabel_loader, test_loader) like the reference's get_ssl_synapse_loader (Synapse.py:135-153)."""
    from .device_pool import DevicePoolLoader
    pool, n = _pool(root, device)
    label_length = int(n * label_num)
    perm = torch.randperm(n).tolist()                     # random_split: randperm(sum(lengths)) from the default generator
    return (DevicePoolLoader(pool, batch_size, train_crop_size, indices=perm[:label_length]),
            DevicePoolLoader(pool, unlabel_batch_size, train_crop_size, indices=perm[label_length:]), _test_loader(root))
