"""Plugin boundary #1: the trainer class nnU-Net discovers BY NAME
(reference utilities/find_class_by_name.py:7-24 walks nnunetv2/training/nnUNetTrainer/**).

Drop this file's class into that tree and ``nnUNetv2_train ... -tr
nnUNetTrainer_MLAgg_2D_dt_MS`` trains the MI355X network with unchanged plans, epoch loop and checkpoints.
nnunetv2 is not importable in the build container (its dependencies are absent offline), so the class
is produced by a factory that receives the base class.

What the class overrides, and why the inherited method cannot stay (B = nnUNetTrainer.py, T = the reference trainer):
  * ``train_step``  B:833-863 runs the network under ``autocast('cuda')`` with a ``GradScaler``.  The MI355X network
                    computes in the precision it was built with (``precision``: "fp32"; "bf16" / "fp16" = 16-bit
                    operands of every Linear and convolution with fp32 sums, i.e. what autocast does to those layers),
                    whatever the ambient autocast state, so the step is ``trainer.train_step`` (zero_grad, forward, loss,
                    backward, clip 12, AdamW).  The ``GradScaler`` of B:152 is kept for "fp16" only (as in the reference,
                    small gradients would otherwise flush to zero in the 16-bit operands) and dropped otherwise;
                    ``loss_scaling="device"`` replaces it with ``trainer.DeviceGradScaler`` (K35: the scaler's decisions on the
                    device, inside the optimizer's launches, so that the fp16 step replays as a hipGraph too); the
                    returned dictionary and the per-step host copy of the loss are the reference's (B:863).
  * ``initialize``  B:193-215 wraps with a plain ``DDP(...)``; here ``trainer.wrap_ddp`` (bucket views, no buffer
                    broadcast) and the loss is rebuilt so that it knows about DDP.
  * ``_build_loss`` T:106-129: the fused Dice + CE deep-supervision loss (K9) with the batch-dice exchange as one
                    all-reduce; the ignore label of partially annotated datasets is handled in K9; region datasets
                    (sigmoid heads, B:330-336) get the fused Dice + BCE loss (K29) on the region planes nnU-Net delivers; a
                    label manager that says ``has_regions`` without naming its ``foreground_regions`` keeps the reference's classes.
                    ``loss=`` of the factories selects one of the reference's loss-variant trainers instead (variants/loss/:
                    top-k cross-entropy on K33, Dice only, CE only, smooth 0): ``trainer.loss_variant_deep_supervision_loss``.
  * ``configure_optimizers``  T:137-147: AdamW + cosine schedule on K11.  ``optimizer=`` of the factories selects the recipe of the
                    reference's base trainer (B:448-452: SGD momentum 0.99 Nesterov + PolyLR) or of its optimizer-variant trainers
                    (variants/optimizer/nnUNetTrainerAdam.py) instead, with the clip and the update fused on the device (K34:
                    ``trainer.ClipSGD`` / ``trainer.ClipAdam`` + ``trainer.PolyLRSchedule``).
  * ``get_dataloaders``  B:566-610, only with ``data_pipeline="device"`` of the factories: the loaders in threads, the base trainer's
                    transform chain on the device (the augmenters, then K36 for the mask, the regions and the deep-supervision levels),
                    batches that arrive on the MI355X (``_device_dataloaders``).  The default inherits the reference's generators.
"""
import contextlib
import math
import os

import numpy as np
import torch

from . import augmentation, augmentation3d, dataloading, evaluation, miopen_tuning, model, trainer

PRECISIONS = ("fp32", "bf16", "fp16")
# The reference loop reads the loss back every step (B:863), so the host cannot run ahead of the device: an eagerly enqueued step then
# costs its ~30 ms of Python / launch time ON TOP of a part of its GPU time (41.6 against 37.7 ms per step at 256 x 256, batch 10:
# profiles/round4_e_bench_with_mfma_roofline.json.log).  After GRAPH_AFTER eager steps on one batch geometry the plugin therefore
# captures the whole step (zero_grad, forward, loss, backward, clip, AdamW: trainer.GraphedTrainStep) and replays it: 38.4 ms with
# the read-back.  Single-process training: fp32 / bf16, and fp16 with loss_scaling="device" (torch's GradScaler reads found_inf on the
# host and cannot be captured); MLAGG_PLUGIN_GRAPH=0 keeps every step eager.
PLUGIN_GRAPH = os.environ.get("MLAGG_PLUGIN_GRAPH", "1") == "1"
GRAPH_AFTER = 3


def _describes_regions(label_manager):
    """A region-based label manager as nnU-Net's LabelManager is one: it names its ``foreground_regions``, one per segmentation head
    (label_handling.py:214-227).  An object that only says ``has_regions`` keeps the reference's own loss classes, its validation
    body and eager steps."""
    regions = getattr(label_manager, "foreground_regions", None)
    return bool(regions) and len(regions) == getattr(label_manager, "num_segmentation_heads", len(regions))


def _region_loss(batch_dice, ddp, ignore_label):
    """The loss of a region-based label manager (reference B:330-352: DeepSupervisionWrapper(DC_and_BCE_loss)): the fused K29 loss on
    the region planes that ConvertSegmentationToRegionsTransform delivers, the ignore plane last when there is an ignore label."""

    def loss(output, target):
        if not isinstance(output, (list, tuple)):                                   # deep supervision off
            output, target = [output], [target if torch.is_tensor(target) else target[0]]
        return trainer.region_deep_supervision_loss(list(output), list(target[:len(output)]), None, batch_dice, ddp,
                                                    ignore_label=ignore_label)

    return loss


DEFAULT_LOSS = "dice_ce"


def _check_loss(loss):
    if loss != DEFAULT_LOSS and loss not in trainer.LOSS_VARIANTS:
        raise RuntimeError(f"loss {loss!r}: {DEFAULT_LOSS!r} or one of {tuple(trainer.LOSS_VARIANTS)}")


def _check_optimizer(optimizer):
    if optimizer is not None and (optimizer == "adamw" or optimizer not in trainer.OPTIMIZERS):
        raise RuntimeError(f"optimizer {optimizer!r}: None (the class's own recipe) or one of {trainer.OPTIMIZERS[1:]}")


LOSS_SCALINGS = ("torch", "device")


def _check_loss_scaling(loss_scaling):
    if loss_scaling not in LOSS_SCALINGS:
        raise RuntimeError(f"loss_scaling {loss_scaling!r}: one of {LOSS_SCALINGS}")


DATA_PIPELINES = ("reference", "device")


def _check_data_pipeline(data_pipeline):
    if data_pipeline not in DATA_PIPELINES:
        raise RuntimeError(f"data_pipeline {data_pipeline!r}: one of {DATA_PIPELINES}")


def _same_ranges(a, b):
    return len(a) == len(b) and all(len(p) == 2 and len(q) == 2 and math.isclose(p[0], q[0], rel_tol=1e-9, abs_tol=1e-12)
                                    and math.isclose(p[1], q[1], rel_tol=1e-9, abs_tol=1e-12) for p, q in zip(a, b))


def _device_dataloaders(self):
    """``get_dataloaders`` (reference B:566-610) of a class built with ``data_pipeline="device"``: the loaders of
    ``get_plain_dataloaders`` (B:612-641) as `dataloading.DataLoader2D` / `DataLoader3D` in worker threads, the transforms of
    ``get_training_transforms`` / ``get_validation_transforms`` (B:644-760) on the device (GpuAugmenter / GpuAugmenter3D, then K36 for
    the mask, the regions and the deep-supervision levels), delivered through `dataloading.PrefetchLoader` with the protocol of the
    reference's generators (`dataloading.DeviceBatchIterator`).  Returns (training iterator, validation iterator).
    The device chain restates the BASE trainer's transforms: a trainer whose ``configure_rotation_dummyDA_mirroring_and_inital_patch_size``
    answers anything else (the DA5, NoDA, DAOrd0, NoMirroring variants) is refused here instead of being trained on another augmentation."""
    cm, lm = self.configuration_manager, self.label_manager
    patch = tuple(int(v) for v in cm.patch_size)
    dim = len(patch)
    ds_scales = self._get_deep_supervision_scales()
    # B:576: also sets self.inference_allowed_mirroring_axes
    rotation_for_DA, dummy_2d, initial_patch_size, mirror_axes = self.configure_rotation_dummyDA_mirroring_and_inital_patch_size()
    got = ([tuple(float(v) for v in rotation_for_DA[k]) for k in ("x", "y", "z")], bool(dummy_2d),
           tuple(int(v) for v in initial_patch_size), None if mirror_axes is None else tuple(int(v) for v in mirror_axes))
    labels = [int(v) for v in lm.all_labels]
    ignore_label = getattr(lm, "ignore_label", None)
    # every value the loaders' segmentation holds: LabelManager.all_labels leaves the ignore label out (label_handling.py:88-102)
    seg_values = labels + ([int(ignore_label)] if ignore_label is not None and int(ignore_label) not in labels else [])
    rank = int(self.local_rank) if self.is_ddp else 0
    seed = getattr(self, "mlagg_data_seed", None)              # None: fresh entropy, as the reference's seeds=None; an int pins every draw
    seed = int(np.random.SeedSequence().entropy % (1 << 30)) if seed is None else int(seed)
    seed += 1000003 * rank
    cascade_labels = None
    if dim == 2:
        rotation = augmentation.rotation_for_2d(patch)
        augmenter = augmentation.GpuAugmenter(patch, self.device, rotation=rotation, mirror_axes=(0, 1), seed=seed, labels=seg_values)
        want = ([tuple(rotation), (0.0, 0.0), (0.0, 0.0)], False, augmenter.initial_patch_size(), (0, 1))
        loader_class = dataloading.DataLoader2D
    elif dim == 3:
        rotation, want_dummy, want_initial, want_mirror = augmentation3d.configure_3d(patch)
        if self.is_cascaded:
            cascade_labels = [int(v) for v in lm.foreground_labels]
        augmenter = augmentation3d.GpuAugmenter3D(patch, self.device, rotation=rotation, mirror_axes=want_mirror, seed=seed,
                                                  labels=seg_values, cascade_labels=cascade_labels, dummy_2d=bool(dummy_2d))
        want = ([tuple(float(v) for v in r) for r in rotation], want_dummy, tuple(want_initial), tuple(want_mirror))
        loader_class = dataloading.DataLoader3D
    else:
        raise RuntimeError(f"data_pipeline='device': a 2-D or 3-D patch, got {patch}")
    if not (_same_ranges(got[0], want[0]) and got[1:] == want[1:]):
        raise RuntimeError("data_pipeline='device' restates the base trainer's training transforms; this trainer asks for (rotation x / y / z, "
                           f"dummy 2-D, initial patch size, mirror axes) = {got}, the device chain would use {want}")
    regions = None
    if getattr(lm, "has_regions", False):
        if not _describes_regions(lm):
            raise RuntimeError("data_pipeline='device': the label manager says has_regions without naming its foreground_regions")
        regions = list(lm.foreground_regions)
    tail = dict(mask_channels=[i for i, m in enumerate(cm.use_mask_for_norm or ()) if m], regions=regions,
                ignore_label=ignore_label)
    levels = dict(ds_scales=ds_scales) if ds_scales is not None else dict(n_levels=1)       # no deep supervision: the map itself

    tr_keys, val_keys = self.do_split()                                             # B:543-564
    previous = self.folder_with_segs_from_previous_stage
    has_ignore = bool(getattr(lm, "has_ignore_label", tail["ignore_label"] is not None))

    def loader(keys, loader_patch):
        dataset = dataloading.Dataset(self.preprocessed_dataset_folder, keys, folder_with_segs_from_previous_stage=previous)
        return loader_class(dataset, self.batch_size, loader_patch, patch, labels, self.oversample_foreground_percent,
                            has_ignore=has_ignore)

    workers = min(max(int(os.environ.get("nnUNet_n_proc_DA", 4)), 1), 16)          # get_allowed_n_proc_DA, at least one thread
    train = dataloading.PrefetchLoader(loader(tr_keys, want[2]), self.device, num_workers=workers, depth=6, seed=seed + 1,
                                       augmenter=augmenter, **levels, **tail)
    try:
        val = dataloading.PrefetchLoader(loader(val_keys, patch), self.device, num_workers=max(1, workers // 2), depth=3,
                                         seed=seed + 500009, cascade_labels=cascade_labels, **levels, **tail)
    except BaseException:
        train.close()
        raise
    self.mlagg_feeds = (dataloading.DeviceBatchIterator(train), dataloading.DeviceBatchIterator(val))
    return self.mlagg_feeds


def _feeds_quiesced(self):
    """The device iterators of `_device_dataloaders` held still (`PrefetchLoader.quiesced`) while the step is captured as a hipGraph."""
    stack = contextlib.ExitStack()
    for feed in getattr(self, "mlagg_feeds", ()):
        stack.enter_context(feed.quiesced())
    return stack


def _variant_optimizers(self, optimizer, capturable):
    """``configure_optimizers`` of a class built with ``optimizer=``: the fused optimizer of that recipe (K34) plus PolyLR over the
    trainer's ``num_epochs``; ``initial_lr`` and ``weight_decay`` are the trainer's (the base trainer's 1e-2 / 3e-5 unless a class set them)."""
    return trainer.configure_optimizers(self.network, getattr(self, "initial_lr", 1e-2), getattr(self, "weight_decay", 3e-5),
                                        capturable=capturable, optimizer=optimizer, num_epochs=int(getattr(self, "num_epochs", 1000)))


def _variant_loss(variant, label_manager, batch_dice, ddp, ignore_label):
    """The loss of one of the reference's loss-variant trainers (variants/loss/nnUNetTrainer{TopkLoss,DiceLoss,CELoss}.py) as
    ``trainer.loss_variant_deep_supervision_loss``.  Region-based label managers: "dice" and "dice_ce_nosmooth" take the fused K29
    loss on the region planes; the top-k and cross-entropy trainers refuse them with the reference's message."""
    regions = bool(getattr(label_manager, "has_regions", False))
    if regions and variant not in ("dice", "dice_ce_nosmooth"):
        raise RuntimeError(trainer.REGIONS_REFUSED)
    if regions and not _describes_regions(label_manager):
        raise RuntimeError(f"loss {variant!r}: the label manager says has_regions without naming its foreground_regions")

    def loss(output, target):
        if not isinstance(output, (list, tuple)):                                   # deep supervision off
            output, target = [output], [target if torch.is_tensor(target) else target[0]]
        return trainer.loss_variant_deep_supervision_loss(list(output), list(target[:len(output)]), variant, batch_dice, ddp,
                                                          ignore_label, regions=regions)

    return loss


def make_trainer_class(nnUNetTrainer, variant="B", precision="fp32", loss=DEFAULT_LOSS, optimizer=None, loss_scaling="torch",
                       data_pipeline="reference"):
    """loss: "dice_ce" (the reference trainer's DC_and_CE_loss / DC_and_BCE_loss) or one of ``trainer.LOSS_VARIANTS`` -- the loss of
    the reference's nnUNetTrainerTopk10Loss ("topk10"), ...Topk10LossLS01 ("topk10_ls01"), ...DiceTopK10Loss ("dice_topk10"),
    ...DiceLoss ("dice"), ...CELoss ("ce") or ...DiceCELoss_noSmooth ("dice_ce_nosmooth").  Every one of them is device-fused, so the
    step is replayed as a hipGraph with any of them; the choice is kept in ``mlagg_loss_variant``.
    optimizer: None (the reference trainer's AdamW + cosine schedule on K11) or the recipe of one of the reference's other trainers on
    K34 with PolyLR: "sgd" (the base trainer's SGD, Nesterov momentum 0.99), "adam" (nnUNetTrainerAdam: AdamW with amsgrad),
    "vanilla_adam" (nnUNetTrainerVanillaAdam: Adam with L2 decay); ``initial_lr`` is then the base trainer's 1e-2.  Every one of them
    keeps its learning rate on the device, so the step replays as a hipGraph too; the choice is kept in ``mlagg_optimizer``.
    loss_scaling: who scales the loss of ``precision="fp16"`` (the other precisions do not scale it).  "torch" (the default): the
    ``torch.amp.GradScaler`` of B:152, eager steps.  "device": ``trainer.DeviceGradScaler`` (K35) with a capturable optimizer -- no host
    synchronisation, no rewrite of the gradients, and the step replays as a hipGraph like every other precision's.  Checkpoints carry
    ``grad_scaler_state`` with torch's keys either way and load into either.  Kept in ``mlagg_loss_scaling``.
    data_pipeline: "reference" (the default) inherits ``get_dataloaders``: batchgenerators worker processes on the CPU (B:566-610).
    "device": `_device_dataloaders` -- the loaders in threads, every transform of the base trainer's chain on the MI355X (the
    augmenters, then K36), batches that arrive on the device.  Kept in ``mlagg_data_pipeline``."""
    if precision not in PRECISIONS:
        raise RuntimeError(f"precision {precision!r}: this build of the MI355X path offers {PRECISIONS}")
    _check_loss(loss)
    _check_optimizer(optimizer)
    _check_loss_scaling(loss_scaling)
    _check_data_pipeline(data_pipeline)
    loss_variant = loss

    class nnUNetTrainer_MLAgg_2D_dt_MS(nnUNetTrainer):
        def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=None):
            super().__init__(plans, configuration, fold, dataset_json, unpack_dataset,
                             device if device is not None else torch.device("cuda"))
            # reference T:52-59
            self.initial_lr = 5e-4 if optimizer is None else 1e-2                   # the base trainer's 1e-2 for its recipes (B:146)
            self.weight_decay = 3e-5
            self.oversample_foreground_percent = 0.33
            self.num_iterations_per_epoch = 250
            self.num_val_iterations_per_epoch = 50
            self.num_epochs = 500
            self.current_epoch = 0
            # B:152 creates a GradScaler for the fp16 autocast of B:848.  fp32 / bf16 do not scale the loss: checkpoints
            # then carry ``grad_scaler_state: None`` exactly as the reference's CPU runs do (B:1018, 1047-1049).
            if precision != "fp16":
                self.grad_scaler = None
            elif loss_scaling == "device" and self.device.type == "cuda":
                self.grad_scaler = trainer.DeviceGradScaler(self.device)            # K35: GradScaler's defaults, decided on the device
            self.mlagg_precision = precision
            self.mlagg_loss_scaling = loss_scaling
            self.mlagg_loss_variant = loss_variant                                  # for logs and checkpoints
            self.mlagg_optimizer = optimizer
            self.mlagg_data_pipeline = data_pipeline
            self._graphed, self._graph_key, self._graph_eager, self._graph_failed = None, None, 0, None
            # run_training.py:123-125 sets cudnn.benchmark (MIOpen's exhaustive find); here: the committed find-db, which
            # holds the fp32 convolutions of the 256 x 256 step only.  Any other patch size or precision takes MIOpen's
            # immediate-mode choice (no find, naive fallback solvers left available): a find-db miss in FAST mode with the
            # naive solvers switched off can stall or end in "no solver found"
            patch = tuple(int(v) for v in self.configuration_manager.patch_size)
            miopen_tuning.use_tuned_convolutions(enabled=(precision == "fp32" and patch == miopen_tuning.TUNED_PATCH))

        @staticmethod
        def build_network_architecture(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                       enable_deep_supervision=True):
            label_manager = plans_manager.get_label_manager(dataset_json)          # reference T:68
            return model.build_network_architecture(configuration_manager.patch_size, num_input_channels,
                                                    label_manager.num_segmentation_heads, enable_deep_supervision,
                                                    variant, precision)

        def initialize(self):                                                       # reference B:193-215
            ddp = self.is_ddp
            self.is_ddp = False           # keeps the inherited body from wrapping with the plain DDP(...) of B:205-207
            try:
                super().initialize()
            finally:
                self.is_ddp = ddp
            if ddp:
                self.network = trainer.wrap_ddp(self.network, self.device.index if self.device.type == "cuda" else None)
                self.loss = self._build_loss()

        def set_deep_supervision_enabled(self, enabled):
            trainer.set_deep_supervision_enabled(self.network, enabled)             # fixes SURVEY finding 7b

        def _get_deep_supervision_scales(self):                                    # reference T:101-104
            return [[1.0 / 2 ** i] * 2 for i in range(5)]

        def _build_loss(self):                                                      # reference T:106-129
            lm = self.label_manager
            batch_dice, ddp = bool(self.configuration_manager.batch_dice), bool(self.is_ddp)
            ignore = getattr(lm, "ignore_label", None)                              # T:116: partially annotated datasets
            if loss_variant != DEFAULT_LOSS:
                return _variant_loss(loss_variant, lm, batch_dice, ddp, ignore)
            if getattr(lm, "has_regions", False):                                   # DC_and_BCE_loss on region planes (T:107-112)
                return _region_loss(batch_dice, ddp, ignore) if _describes_regions(lm) else super()._build_loss()

            def loss(output, target):
                if not isinstance(output, (list, tuple)):                           # deep supervision off (validation of
                    output, target = [output], [target if torch.is_tensor(target) else target[0]]   # a no-DS network)
                return trainer.deep_supervision_loss(list(output), list(target[:len(output)]), batch_dice, ddp,
                                                     ignore_label=ignore)

            return loss

        def _graph_ok(self):
            """The step may be replayed as a hipGraph: one process, no torch GradScaler (its step reads found_inf on the host; a
            DeviceGradScaler is captured with the step), the fused device loss, a device network."""
            lm = self.label_manager
            scaler_ok = self.grad_scaler is None or isinstance(self.grad_scaler, trainer.DeviceGradScaler)
            return bool(PLUGIN_GRAPH and self._graph_failed is None and not self.is_ddp and scaler_ok
                        and self.device.type == "cuda" and (not getattr(lm, "has_regions", False) or _describes_regions(lm)))

        def configure_optimizers(self):                                             # reference T:137-147
            # capturable: learning rate and step counter live on the device, so the same optimizer serves eager and replayed steps.  A
            # DeviceGradScaler needs that form whether or not the step is replayed (MLAGG_PLUGIN_GRAPH=0, DDP, a region dataset the
            # fused loss does not describe): only the device step counter can leave a skipped step uncounted without a synchronisation
            capturable = self._graph_ok() or isinstance(self.grad_scaler, trainer.DeviceGradScaler)
            if optimizer is not None:
                return _variant_optimizers(self, optimizer, capturable)
            return trainer.configure_optimizers(self.network, self.initial_lr, self.weight_decay, capturable=capturable)

        if data_pipeline == "device":
            get_dataloaders = _device_dataloaders                                   # reference B:566-610

        def _to_device(self, batch):                                                # reference B:834-841
            data = batch["data"].to(self.device, non_blocking=True)
            target = batch["target"]
            target = [t.to(self.device, non_blocking=True) for t in target] if isinstance(target, list) else \
                target.to(self.device, non_blocking=True)
            return data, target

        def train_step(self, batch):                                                # reference B:833-863
            data, target = self._to_device(batch)
            if not isinstance(target, list):
                target = [target]
            data, target = data.float(), [t.float() for t in target]
            if self._graph_ok() and isinstance(self.optimizer, trainer.ClipOptimizer) and self.optimizer.capturable:
                key = (tuple(data.shape),) + tuple(tuple(t.shape) for t in target)
                if self._graphed is not None and key == self._graph_key:
                    return {"loss": self._graphed(data, target).cpu().numpy()}      # replay + the reference's per-step host copy
                if self._graphed is None:
                    self._graph_eager = self._graph_eager + 1 if key == self._graph_key else 1
                    self._graph_key = key
                    if self._graph_eager > GRAPH_AFTER:
                        try:
                            # warmup=0: the eager steps above were the warm-up; the capture itself executes nothing, so the first
                            # replay IS this step (no batch is trained on twice)
                            with _feeds_quiesced(self):                             # no loader thread calls the runtime meanwhile
                                self._graphed = trainer.GraphedTrainStep(self.network, self.optimizer, data, target, clip=12.0,
                                                                         warmup=0, loss_fn=self.loss, grad_scaler=self.grad_scaler)
                            return {"loss": self._graphed().cpu().numpy()}
                        except Exception as e:                                      # noqa: BLE001  (stay eager, say why once)
                            self._graphed, self._graph_failed = None, repr(e)
                            self.print_to_log_file(f"MLAgg: hipGraph capture of the train step failed ({e!r}); steps stay eager")
            loss = trainer.train_step(self.network, self.optimizer, data, target, clip=12.0, loss_fn=self.loss,
                                      grad_scaler=self.grad_scaler)
            return {"loss": loss.cpu().numpy()}                                     # the reference's per-step host copy

        def validation_step(self, batch):                                           # reference B:880-942
            lm = self.label_manager
            if getattr(lm, "has_regions", False) and not _describes_regions(lm):
                return super().validation_step(batch)        # the reference's loss classes: the reference's own body too
            data, target = self._to_device(batch)
            # B:897 evaluates self.loss; B:917-929 masks the ignore label out of tp / fp / fn; sigmoid regions: B:906-907, 920-923
            return evaluation.validation_step(self.network, data, target, self.configuration_manager.batch_dice,
                                              self.is_ddp, getattr(self.label_manager, "ignore_label", None), self.loss,
                                              regions=bool(getattr(self.label_manager, "has_regions", False)))

        def on_validation_epoch_end(self, val_outputs):                             # reference B:944-978
            res = evaluation.validation_epoch_end(val_outputs)
            for key in ("mean_fg_dice", "dice_per_class_or_region", "val_losses"):
                self.logger.log(key, res[key], self.current_epoch)

        def plot_network_architecture(self):
            pass

    return nnUNetTrainer_MLAgg_2D_dt_MS


def make_umamba_enc_ss3d_trainer_class(nnUNetTrainer, loss=DEFAULT_LOSS, optimizer=None, loss_scaling="torch",
                                       data_pipeline="reference"):
    """``nnUNetTrainerUMambaEnc_SS3D`` (reference variants/mamba/nnUNetTrainerUMambaEnc_SS3D.py:8-31) on the MI355X 3-D network
    (model3d.UMambaEnc; BASELINE configs[3]).  The reference class overrides ``build_network_architecture`` only and inherits the
    base trainer's recipe (SGD momentum 0.99 Nesterov + PolyLR, nnUNetTrainer.py:448-452; DC_and_CE deep-supervision loss,
    :330-352); so does this one, plus what the device network needs from the loop: the fp32 step without autocast / GradScaler
    (B:848-858), the fused K9 loss, ``trainer.wrap_ddp``, and the deep-supervision switch on the unwrapped module.
    loss: as in ``make_trainer_class``.
    optimizer: None inherits the host trainer's ``configure_optimizers`` (torch.optim.SGD behind clip_grad_norm_); "sgd" is the same
    recipe with the clip and the update fused on the device (K34: ClipSGD + PolyLR), i.e. the reference's class with its step tail on
    the MI355X; "adam" / "vanilla_adam" as in ``make_trainer_class``.  The 3-D step stays eager.  Kept in ``mlagg_optimizer``.
    loss_scaling: as in ``make_trainer_class``; the 3-D network computes in fp32 and scales no loss, so the choice is checked, kept in
    ``mlagg_loss_scaling`` and has no further effect.
    data_pipeline: as in ``make_trainer_class`` (3-D: GpuAugmenter3D with the dummy-2-D and cascade chains where the plan asks for them)."""
    from . import model3d
    _check_loss(loss)
    _check_optimizer(optimizer)
    _check_loss_scaling(loss_scaling)
    _check_data_pipeline(data_pipeline)
    loss_variant = loss

    class nnUNetTrainerUMambaEnc_SS3D(nnUNetTrainer):
        def __init__(self, plans, configuration, fold, dataset_json, unpack_dataset=True, device=None):
            super().__init__(plans, configuration, fold, dataset_json, unpack_dataset,
                             device if device is not None else torch.device("cuda"))
            self.grad_scaler = None                                                  # fp32 step: no loss scaling (B:152)
            self.mlagg_loss_variant = loss_variant                                   # for logs and checkpoints
            self.mlagg_optimizer = optimizer
            self.mlagg_loss_scaling = loss_scaling
            self.mlagg_data_pipeline = data_pipeline
            miopen_tuning.use_tuned_convolutions(enabled=False)                      # no committed records for 3-D convolutions

        @staticmethod
        def build_network_architecture(plans_manager, dataset_json, configuration_manager, num_input_channels,
                                       enable_deep_supervision=True):
            cm = configuration_manager                                               # get_umamba_enc_3d_from_plans, S:890-942
            if len(cm.conv_kernel_sizes[0]) != 3:
                raise RuntimeError("nnUNetTrainerUMambaEnc_SS3D on MI355X: 3-D configurations only")
            label_manager = plans_manager.get_label_manager(dataset_json)
            return model3d.build_network_architecture_3d(
                num_input_channels, label_manager.num_segmentation_heads, cm.conv_kernel_sizes, cm.pool_op_kernel_sizes,
                cm.n_conv_per_stage_encoder, cm.n_conv_per_stage_decoder, cm.UNet_base_num_features, cm.unet_max_num_features,
                enable_deep_supervision)

        def initialize(self):                                                        # reference B:193-215
            ddp = self.is_ddp
            self.is_ddp = False
            try:
                super().initialize()
            finally:
                self.is_ddp = ddp
            if ddp:
                self.network = trainer.wrap_ddp(self.network, self.device.index if self.device.type == "cuda" else None)
                self.loss = self._build_loss()

        def set_deep_supervision_enabled(self, enabled):                             # B: self.network.decoder.deep_supervision
            trainer.set_deep_supervision_enabled(self.network, enabled)

        def _build_loss(self):                                                       # reference B:330-352
            lm = self.label_manager
            batch_dice, ddp = bool(self.configuration_manager.batch_dice), bool(self.is_ddp)
            ignore = getattr(lm, "ignore_label", None)
            if loss_variant != DEFAULT_LOSS:
                return _variant_loss(loss_variant, lm, batch_dice, ddp, ignore)
            if getattr(lm, "has_regions", False):
                return _region_loss(batch_dice, ddp, ignore) if _describes_regions(lm) else super()._build_loss()

            def loss(output, target):
                if not isinstance(output, (list, tuple)):
                    output, target = [output], [target if torch.is_tensor(target) else target[0]]
                return trainer.deep_supervision_loss(list(output), list(target[:len(output)]), batch_dice, ddp, ignore_label=ignore)

            return loss

        if data_pipeline == "device":
            get_dataloaders = _device_dataloaders                                    # reference B:566-610

        if optimizer is not None:
            def configure_optimizers(self):                                          # reference B:448-452 / nnUNetTrainerAdam.py
                return _variant_optimizers(self, optimizer, False)                   # the 3-D step is not captured

        def train_step(self, batch):                                                 # reference B:833-863
            data = batch["data"].to(self.device, non_blocking=True)
            target = batch["target"]
            target = [t.to(self.device, non_blocking=True) for t in target] if isinstance(target, list) else \
                [target.to(self.device, non_blocking=True)]
            loss = trainer.train_step(self.network, self.optimizer, data.float(), [t.float() for t in target], clip=12.0,
                                      loss_fn=self.loss)
            return {"loss": loss.cpu().numpy()}

        def plot_network_architecture(self):
            pass

    return nnUNetTrainerUMambaEnc_SS3D
