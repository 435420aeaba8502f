"""Generate tests/golden/dataloader_3d.npz from the REFERENCE's own nnUNetDataLoader3D.

    MLAGG_REFERENCE=<reference checkout> python tests/golden/make_golden_dataloader_3d.py

training/dataloading/data_loader_3d.py, base_data_loader.py and nnunet_dataset.py are imported unmodified; the stand-ins are
those of make_golden.py:golden_dataloader (batchgenerators' DataLoader with its get_indices for infinite=True restated, the
file helpers, LabelManager).  Three seeded batches per setting of tests/_dataloading_3d_cases.CASES on its synthetic case
folders.  Only the data is committed."""
import importlib
import os
import pickle
import sys
import tempfile
import types
import typing

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "MLAGG_REFERENCE" not in os.environ:
    raise SystemExit("set MLAGG_REFERENCE to a checkout of the reference repository (aticejiang/MLAgg-UNet)")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.environ["MLAGG_REFERENCE"], "mlagg"))

from tests import _dataloading_3d_cases as K  # noqa: E402


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class DataLoader:
    def __init__(self, data, batch_size, num_threads_in_multithreaded=1, seed_for_shuffle=None, return_incomplete=False,
                 shuffle=True, infinite=False, sampling_probabilities=None):
        self._data, self.batch_size, self.infinite = data, batch_size, infinite
        self.sampling_probabilities, self.indices = sampling_probabilities, None

    def get_indices(self):
        assert self.infinite
        return np.random.choice(self.indices, self.batch_size, replace=True, p=self.sampling_probabilities)


def load_pickle(f):
    with open(f, "rb") as fh:
        return pickle.load(fh)


def main():
    _mod("batchgenerators")
    _mod("batchgenerators.dataloading")
    _mod("batchgenerators.dataloading.data_loader", DataLoader=DataLoader)
    _mod("batchgenerators.utilities")
    _mod("batchgenerators.utilities.file_and_folder_operations", join=os.path.join, isfile=os.path.isfile,
         load_pickle=load_pickle, subfiles=None, List=typing.List, os=os)
    _mod("nnunetv2.configuration", default_num_processes=1)
    _mod("nnunetv2.utilities.label_handling")
    _mod("nnunetv2.utilities.label_handling.label_handling", LabelManager=object)
    D3 = importlib.import_module("nnunetv2.training.dataloading.data_loader_3d")
    DS = importlib.import_module("nnunetv2.training.dataloading.nnunet_dataset")

    class LM:
        all_labels = K.LABELS
        has_ignore_label = False

    class LMIgnore(LM):
        has_ignore_label = True

    out = {}
    for tag, (unpack, patch, final, bs, fg) in K.CASES.items():
        folder = tempfile.mkdtemp()
        K.write_dataset_3d(folder, unpack=unpack, ignore_label=4 if tag == "ign" else None)
        dl = D3.nnUNetDataLoader3D(DS.nnUNetDataset(folder), bs, patch, final, LMIgnore() if tag == "ign" else LM(),
                                   oversample_foreground_percent=fg, sampling_probabilities=None, pad_sides=None)
        np.random.seed(11)
        for it in range(3):
            b = dl.generate_train_batch()
            out[f"{tag}_data_{it}"] = b["data"]
            out[f"{tag}_seg_{it}"] = b["seg"]
            out[f"{tag}_keys_{it}"] = np.asarray([str(k) for k in b["keys"]])
    np.savez_compressed(os.path.join(HERE, "dataloader_3d.npz"), **out)
    print("dataloader_3d", {k: v.shape for k, v in out.items() if k.endswith("_0")})


if __name__ == "__main__":
    main()
