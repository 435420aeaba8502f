"""CPU: ``data_pipeline="device"`` of both trainer factories behind the stand-in base class (tests/fake_nnunet_data.py): the
get_dataloaders override (reference nnUNetTrainer.py:566-610) end to end on CPU tensors, where ops.batch_tail is its host composition."""
import pytest
import torch

import fake_nnunet as FK
import fake_nnunet_data as FD
import _data_pipeline_cases as P


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pipeline"))


@pytest.mark.parametrize("kind", list(P.KINDS))
def test_device_pipeline_delivers_the_reference_chain(kind, root, monkeypatch):
    P.check_pipeline(kind, P.write_folder(root, kind), "cpu", monkeypatch)


def test_reference_pipeline_is_the_inherited_one_and_the_choice_is_checked(root):
    from mlagg_unet_amd import nnunet_plugin
    desc = P.write_folder(root, "2d")
    base = FD.with_data(**desc)
    for kind in ("2d", "3d"):
        default = P.trainer_class(kind, desc, data_pipeline="reference", base=base)
        assert default.get_dataloaders is base.get_dataloaders
        assert P.trainer_class(kind, desc, base=base).get_dataloaders is nnunet_plugin._device_dataloaders
    tr = nnunet_plugin.make_trainer_class(base)(FK.make_plans((32, 48), 2), "2d_bs10", 0, FK.make_dataset_json(4), device=torch.device("cpu"))
    assert tr.mlagg_data_pipeline == "reference" and tr.get_dataloaders() == "reference-generators" and tr.base_calls["get_dataloaders"] == 1
    for factory in (nnunet_plugin.make_trainer_class, nnunet_plugin.make_umamba_enc_ss3d_trainer_class):
        with pytest.raises(RuntimeError):
            factory(base, data_pipeline="gpu")


def test_another_augmentation_or_unnamed_regions_are_refused(root, monkeypatch):
    """The device chain restates the base trainer's transforms only: a trainer that configures another rotation, mirroring or initial
    patch size (the DA5 / NoMirroring / NoDA variants do) fails loudly, and so does a region label manager without its regions."""
    import threading
    monkeypatch.setenv("nnUNet_n_proc_DA", "1")
    desc = P.write_folder(root, "2d")
    before = threading.active_count()

    def variant(change):
        class Variant(FD.with_data(**desc)):
            def configure_rotation_dummyDA_mirroring_and_inital_patch_size(self):
                return change(*super().configure_rotation_dummyDA_mirroring_and_inital_patch_size())
        return Variant

    changes = [lambda rot, dummy, initial, mirror: (rot, dummy, initial, None),                                   # NoMirroring
               lambda rot, dummy, initial, mirror: (rot, dummy, tuple(P.KINDS["2d"][1]), mirror),                 # NoDA: the final patch
               lambda rot, dummy, initial, mirror: (dict(rot, x=(-0.5, 0.5)), dummy, initial, mirror),
               lambda rot, dummy, initial, mirror: (rot, True, initial, mirror)]
    for change in changes:
        tr = P.make_trainer("2d", desc, "cpu", base=variant(change))
        with pytest.raises(RuntimeError, match="device chain"):
            tr.get_dataloaders()
    unnamed = dict(P.write_folder(root, "2d_regions_mask"), name_regions=False)
    tr = P.make_trainer("2d_regions_mask", unnamed, "cpu")
    with pytest.raises(RuntimeError, match="foreground_regions"):
        tr.get_dataloaders()
    assert threading.active_count() == before                                  # a refused call leaves no worker behind


def test_worker_count_follows_the_environment(root, monkeypatch):
    desc = P.write_folder(root, "2d")
    for value, want in (("3", (3, 1)), ("0", (1, 1)), ("40", (16, 8))):
        monkeypatch.setenv("nnUNet_n_proc_DA", value)
        train_it, val_it = P.make_trainer("2d", desc, "cpu").get_dataloaders()
        try:
            assert (len(train_it.loader.workers), len(val_it.loader.workers)) == want
        finally:
            train_it._finish()
            val_it._finish()
        assert not any(t.is_alive() for it in (train_it, val_it) for t in it.loader.workers)
