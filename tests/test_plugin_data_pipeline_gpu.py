"""GPU: ``data_pipeline="device"`` on the MI355X: the batches of get_dataloaders() (K36 behind the augmenters, on the loader's side
stream) equal the hand-composed chain bit for bit, and the plugin's train / validation steps run on them, the hipGraph replay included."""
import numpy as np
import pytest
import torch

import _data_pipeline_cases as P

pytestmark = pytest.mark.gpu
IMG = (64, 64)                          # the smallest patch the plugin's GPU tests build the 2-D network at


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pipeline_gpu"))


@pytest.mark.parametrize("kind", list(P.KINDS))
def test_device_pipeline_delivers_the_reference_chain(kind, root, monkeypatch):
    P.check_pipeline(kind, P.write_folder(root, kind), "cuda", monkeypatch)


@pytest.mark.parametrize("kind", ["2d", "2d_regions_mask"])
def test_train_and_validation_steps_fed_from_the_iterators(kind, root, monkeypatch):
    """Two train steps and a validation step on batches of the device iterators return finite losses; after GRAPH_AFTER + 1 steps on
    the one geometry the iterator delivers, the step is a replayed hipGraph."""
    from mlagg_unet_amd import nnunet_plugin
    from oracle import mlagg_oracle as O
    monkeypatch.setenv("nnUNet_n_proc_DA", "2")
    tr = P.make_trainer(kind, P.write_folder(root, kind), "cuda", patch=IMG)
    tr.initialize()
    O.deterministic_fill_(tr.network.state_dict())
    assert nnunet_plugin.PLUGIN_GRAPH and tr._graph_ok()
    train_it, val_it = tr.get_dataloaders()
    try:
        for step in range(nnunet_plugin.GRAPH_AFTER + 1):
            batch = next(train_it)
            assert batch["data"].is_cuda and all(t.is_cuda for t in batch["target"])
            out = tr.train_step(batch)
            assert isinstance(out["loss"], np.ndarray) and np.isfinite(out["loss"]), step
            if step == 1:
                val = tr.validation_step(next(val_it))
                assert bool(torch.isfinite(torch.as_tensor(val["loss"])).all()) and set(val) >= {"tp_hard", "fp_hard", "fn_hard"}
        assert tr._graphed is not None and tr._graph_failed is None
        assert tr.base_calls["train_step"] == 0 and tr.base_calls["get_dataloaders"] == 0
    finally:
        train_it._finish()
        val_it._finish()
    assert not any(t.is_alive() for it in (train_it, val_it) for t in it.loader.workers)
