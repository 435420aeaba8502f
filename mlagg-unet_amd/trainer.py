"""Train step, loss and data-parallel wiring of ``nnUNetTrainer_MLAgg_2D_dt_MS`` for MI355X.

Mirrors the reference's trainer surface on the hot path:
  * ``train_step``            reference nnUNetTrainer.py:833-863 (fp32 branch: zero_grad, forward, loss,
                              backward, clip_grad_norm_ 12, optimizer step)
  * ``configure_optimizers``  reference nnUNetTrainer_MLAgg_2D_dt_MS.py:137-147 (AdamW 5e-4 / 3e-5 / eps 1e-4,
                              timm CosineLRScheduler restated: t_initial 500, lr_min 1e-6, warmup 10 @ 1e-4)
                              and, by ``optimizer=``, the base trainer's SGD + PolyLR (nnUNetTrainer.py:448-452) and the Adam
                              recipes of variants/optimizer/nnUNetTrainerAdam.py: ``ClipSGD`` / ``ClipAdam`` (K34), ``PolyLRSchedule``
  * ``deep_supervision_loss`` reference loss/deep_supervision.py:17-34 over DC_and_CE_loss
                              (loss/compound_losses.py:31-57, loss/dice.py:73-117, loss/robust_ce_loss.py:12-16)
  * ``region_deep_supervision_loss``  the same wrapper over DC_and_BCE_loss (loss/compound_losses.py:60-100), the loss of
                              region-based datasets with sigmoid heads (nnUNetTrainer.py:330-336)
  * ``loss_variant_deep_supervision_loss``  the wrapper over the losses of the loss-variant trainers (variants/loss/: TopKLoss,
                              DC_and_topk_loss, Dice alone, cross-entropy alone, Dice + CE with smooth 0)
  * ``wrap_ddp``              reference nnUNetTrainer.py:205-207, without its ``dummy_tensor`` hazard
  * ``split_batch_size``      reference nnUNetTrainer.py:283-328 with the zero/negative per-rank sizes fixed (7c)
One process per GPU; ``torch.distributed`` backend "nccl" is RCCL on ROCm (xGMI inside a node).
"""
import math
import os
from typing import List

import torch
import torch.distributed as dist
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------
class _AllGatherSum(torch.autograd.Function):
    """Sum over ranks of a small statistics tensor.  Equivalent to the reference's
    AllGatherGrad(...).sum(0) (utilities/ddp_allgather.py:25-48 used at loss/dice.py:104-107) --
    forward: sum of every rank's statistics; backward: the SUM over ranks of the upstream gradients
    (reference :46 all_reduce then [rank] slice), which DDP's gradient averaging then turns into the
    gradient of the global-batch dice -- but as ONE all-reduce each way for the three dice statistics
    instead of three all_gathers forward + three all_reduces backward per deep-supervision level."""

    @staticmethod
    def forward(ctx, stats):
        out = stats.clone()
        dist.all_reduce(out, op=dist.ReduceOp.SUM)
        return out

    @staticmethod
    def backward(ctx, grad):
        g = grad.clone()
        dist.all_reduce(g, op=dist.ReduceOp.SUM)
        return g


def soft_dice_loss(logits, target, batch_dice=True, smooth=1e-5, ddp=False, mask=None):
    """MemoryEfficientSoftDiceLoss (loss/dice.py:73-117), do_bg False; `mask` (B, 1, ...) bool: the loss mask of an ignore label."""
    probs = logits.softmax(1)[:, 1:]
    axes = tuple(range(2, logits.ndim))
    with torch.no_grad():
        onehot = torch.zeros(logits.shape, dtype=torch.bool, device=logits.device)
        onehot.scatter_(1, target.long(), 1)
        onehot = onehot[:, 1:]
        if mask is not None:
            onehot = onehot & mask
        sum_gt = onehot.sum(axes).to(probs.dtype)
    intersect = (probs * onehot).sum(axes)
    sum_pred = (probs if mask is None else probs * mask).sum(axes)
    if batch_dice:
        stats = torch.stack([intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)])
        if ddp:
            stats = _AllGatherSum.apply(stats)
        intersect, sum_pred, sum_gt = stats[0], stats[1], stats[2]
    dc = (2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)
    return -dc.mean()


def dc_and_ce_loss(logits, target, batch_dice=True, ddp=False, ignore_label=None):
    """DC_and_CE_loss.forward (loss/compound_losses.py:31-57) incl. its ignore-label branch (:38-50)."""
    if ignore_label is None:
        return F.cross_entropy(logits, target[:, 0].long()) + soft_dice_loss(logits, target, batch_dice, ddp=ddp)
    mask = target != ignore_label
    target_dice = torch.where(mask, target, torch.zeros_like(target))
    dc = soft_dice_loss(logits, target_dice, batch_dice, ddp=ddp, mask=mask)
    if int(mask.sum()) == 0:                            # the reference skips the cross-entropy of a fully ignored batch
        return dc
    return F.cross_entropy(logits, target[:, 0].long(), ignore_index=int(ignore_label)) + dc


def deep_supervision_weights(n=5):
    w = [1.0 / 2 ** i for i in range(n)]
    s = sum(w)
    return [v / s for v in w]


def deep_supervision_loss_eager(outputs, targets, batch_dice=True, ddp=False, ignore_label=None):
    """The loss as the reference composes it, level by level in torch ops (host tensors / CPU tests)."""
    ws = deep_supervision_weights(len(outputs))
    total = ws[0] * dc_and_ce_loss(outputs[0], targets[0], batch_dice, ddp, ignore_label)
    for w, o, t in zip(ws[1:], outputs[1:], targets[1:]):
        total = total + w * dc_and_ce_loss(o, t, batch_dice, ddp, ignore_label)
    return total


_LEVEL_CONSTANTS = {}


def _level_constants(npix, device):
    """Per-level weight / pixel count (cross-entropy mean) and weight (dice) as device tensors, uploaded once."""
    key = (npix, str(device))
    if key not in _LEVEL_CONSTANTS:
        w = deep_supervision_weights(len(npix))
        _LEVEL_CONSTANTS[key] = (torch.tensor([wi / n for wi, n in zip(w, npix)], device=device, dtype=torch.float32),
                                 torch.tensor(w, device=device, dtype=torch.float32))
    return _LEVEL_CONSTANTS[key]


def deep_supervision_loss(outputs, targets, batch_dice=True, ddp=False, smooth=1e-5, ignore_label=None):
    """DeepSupervisionWrapper(DC_and_CE_loss) of reference T:106-129.  On the MI355X: K9 reads every logit map once
    for the statistics and once for the gradient (2 x 5 kernels instead of ~310 launches, 2.5 -> 0.3 ms at config 2);
    the (levels, classes)-sized algebra below is torch, vectorised over the levels, and the batch-dice statistics of
    all levels cross the ranks in ONE all-reduce each way."""
    if not outputs[0].is_cuda:
        return deep_supervision_loss_eager(outputs, targets, batch_dice, ddp, ignore_label)
    from . import ops
    ip, gt, ce = ops.dice_ce_stats(list(outputs), list(targets), ignore_label)   # (L, B, 2, C), (L, B, C), (L,)
    inter, pred, gts = ip[:, :, 0, 1:], ip[:, :, 1, 1:], gt[:, :, 1:]        # background dropped (do_bg=False)
    if batch_dice:
        stats = torch.stack([inter.sum(1), pred.sum(1), gts.sum(1)])        # (3, L, C-1)
        if ddp:
            stats = _AllGatherSum.apply(stats)
        inter, pred, gts = stats[0], stats[1], stats[2]
    dc = (2 * inter + smooth) / torch.clip(gts + pred + smooth, 1e-8)
    dice = -dc.flatten(1).mean(1)                                           # (L,)
    w_ce, w_dice = _level_constants(tuple(o.numel() // o.shape[1] for o in outputs), ce.device)
    if ignore_label is not None:
        # cross-entropy mean over the pixels that are NOT ignored (CrossEntropyLoss(ignore_index), local to the rank as in the
        # reference); every valid pixel hits exactly one class, so their number is the sum of the label counts.  A fully ignored
        # level has ce = 0 and contributes nothing, like the reference's `num_fg > 0` test
        w_ce = w_dice / gt.sum((1, 2)).clamp(min=1.0)
    return (w_ce * ce + w_dice * dice).sum()


# ------------------------------------------------------------------------------------------------
# loss variants (reference training/nnUNetTrainer/variants/loss)
# ------------------------------------------------------------------------------------------------
# variant -> (top-k percent or None, label smoothing, Dice term, cross-entropy term, Dice smooth)
LOSS_VARIANTS = {
    "topk10": (10, 0.0, False, False, None),              # nnUNetTrainerTopk10Loss: TopKLoss(k=10)
    "topk10_ls01": (10, 0.1, False, False, None),         # nnUNetTrainerTopk10LossLS01: TopKLoss(k=10, label_smoothing=0.1)
    "dice_topk10": (10, 0.0, True, False, 1e-5),          # nnUNetTrainerDiceTopK10Loss: DC_and_topk_loss, SoftDiceLoss, weights 1 / 1
    "dice": (None, 0.0, True, False, 1e-5),               # nnUNetTrainerDiceLoss: MemoryEfficientSoftDiceLoss alone
    "ce": (None, 0.0, False, True, None),                 # nnUNetTrainerCELoss: RobustCrossEntropyLoss
    "dice_ce_nosmooth": (None, 0.0, True, True, 0.0),     # nnUNetTrainerDiceCELoss_noSmooth: DC_and_CE_loss with smooth 0
}
REGIONS_REFUSED = "regions not supported by this trainer"        # the reference's assertion message (nnUNetTrainerTopkLoss.py:10)


def _loss_variant(variant):
    if variant not in LOSS_VARIANTS:
        raise RuntimeError(f"loss variant {variant!r}: one of {tuple(LOSS_VARIANTS)}")
    return LOSS_VARIANTS[variant]


def topk_loss(logits, target, kpercent=10, ignore_label=None, label_smoothing=0.0):
    """TopKLoss.forward (loss/robust_ce_loss.py:27-32) in torch ops, one level: the mean of the k largest per-pixel cross-entropies,
    k = int(N kpercent / 100) of ALL N pixels; ignored pixels have the value 0.  k == 0 raises (the reference returns NaN)."""
    from . import ops
    ce = F.cross_entropy(logits, target[:, 0].long(), reduction="none", ignore_index=-100 if ignore_label is None else int(ignore_label),
                         label_smoothing=label_smoothing)
    return torch.topk(ce.reshape(-1), ops.topk_count(ce.numel(), kpercent), sorted=False)[0].mean()


def loss_variant_level_eager(logits, target, variant, batch_dice=True, ddp=False, ignore_label=None):
    """One level of a loss variant as the reference composes it, in torch ops."""
    kpercent, eps, with_dice, with_ce, smooth = _loss_variant(variant)
    if variant == "dice":                                   # nnUNetTrainerDiceLoss passes no loss mask: the ignore label plays no part
        return soft_dice_loss(logits, target, batch_dice, smooth, ddp)
    total = None
    if with_dice:                                           # the ignore branch of DC_and_CE_loss / DC_and_topk_loss (compound_losses.py:38-50)
        if ignore_label is None:
            total = soft_dice_loss(logits, target, batch_dice, smooth, ddp)
        else:
            mask = target != ignore_label
            total = soft_dice_loss(logits, torch.where(mask, target, torch.zeros_like(target)), batch_dice, smooth, ddp, mask)
    if ignore_label is not None and int((target != ignore_label).sum()) == 0:
        # nothing to classify: DC_and_CE_loss / DC_and_topk_loss skip the term (`num_fg > 0`); so do the pure variants here, where
        # the reference's CrossEntropyLoss gives NaN (mean over no pixel) and its TopKLoss 0
        return total if total is not None else logits.sum() * 0.0
    if kpercent is not None:
        term = topk_loss(logits, target, kpercent, ignore_label, eps)
    else:
        term = F.cross_entropy(logits, target[:, 0].long(), ignore_index=-100 if ignore_label is None else int(ignore_label))
    return term if total is None else term + total


def loss_variant_deep_supervision_loss_eager(outputs, targets, variant, batch_dice=True, ddp=False, ignore_label=None):
    """A loss variant under the DeepSupervisionWrapper, level by level in torch ops, ``torch.topk`` included (host tensors, CPU tests)."""
    ws = deep_supervision_weights(len(outputs))
    total = None
    for w, o, t in zip(ws, outputs, targets):
        level = w * loss_variant_level_eager(o, t, variant, batch_dice, ddp, ignore_label)
        total = level if total is None else total + level
    return total


def _dice_levels(ip, gt, batch_dice, ddp, smooth):
    """-mean dice per level (L,) from K9's statistics, background dropped; batch dice crosses the ranks in one all-reduce each way."""
    inter, pred, gts = ip[:, :, 0, 1:], ip[:, :, 1, 1:], gt[:, :, 1:]
    if batch_dice:
        stats = torch.stack([inter.sum(1), pred.sum(1), gts.sum(1)])        # (3, L, C-1)
        if ddp:
            stats = _AllGatherSum.apply(stats)
        inter, pred, gts = stats[0], stats[1], stats[2]
    dc = (2 * inter + smooth) / torch.clip(gts + pred + smooth, 1e-8)
    return -dc.flatten(1).mean(1)


def loss_variant_deep_supervision_loss(outputs, targets, variant, batch_dice=True, ddp=False, ignore_label=None, regions=False):
    """The losses of the reference's loss-variant trainers (variants/loss/nnUNetTrainer{TopkLoss,DiceLoss,CELoss}.py) under the
    DeepSupervisionWrapper, weights ``deep_supervision_weights``.  variant:
      "topk10"            nnUNetTrainerTopk10Loss          TopKLoss(k=10): mean of the 10 % largest per-pixel cross-entropies
      "topk10_ls01"       nnUNetTrainerTopk10LossLS01      ... with label smoothing 0.1
      "dice_topk10"       nnUNetTrainerDiceTopK10Loss      DC_and_topk_loss: SoftDiceLoss (do_bg False, smooth 1e-5) + TopKLoss, weights 1 / 1;
                                                           the Dice statistics cross the ranks, the top-k is local to the rank
      "dice"              nnUNetTrainerDiceLoss            MemoryEfficientSoftDiceLoss alone (no loss mask: ignore_label plays no part)
      "ce"                nnUNetTrainerCELoss              RobustCrossEntropyLoss
      "dice_ce_nosmooth"  nnUNetTrainerDiceCELoss_noSmooth DC_and_CE_loss with smooth 0
    On the MI355X the top-k variants run K33 (per level one pass for the per-pixel values and the Dice statistics, an exact radix
    select of the k-th largest value, one gradient pass); the others are K9's statistics plus algebra.  All of them are device-fused
    and record into a hipGraph.  k = int(N 10 / 100) counts ignored pixels, as the reference does; k == 0 raises where the reference
    returns NaN; pixels that tie with the k-th value share the remaining weight equally (``torch.topk`` picks among them in an
    unspecified order: the value is the same, the gradient of the tied pixels may differ).  A level without a valid pixel contributes
    no cross-entropy term.  CPU tensors take ``loss_variant_deep_supervision_loss_eager``.
    regions: False for label datasets.  For region-based datasets (sigmoid heads) True when the targets are region planes, or the label
    manager's ``foreground_regions`` when they are label maps: "dice" and "dice_ce_nosmooth" then go through
    ``region_deep_supervision_loss``; the other variants refuse regions as the reference's trainers do."""
    kpercent, eps, with_dice, with_ce, smooth = _loss_variant(variant)
    if regions is not False and regions is not None:
        if variant not in ("dice", "dice_ce_nosmooth"):
            raise RuntimeError(REGIONS_REFUSED)
        return region_deep_supervision_loss(outputs, targets, None if regions is True else regions, batch_dice, ddp, smooth, ignore_label,
                                            weight_ce=1.0 if with_ce else 0.0)
    if not outputs[0].is_cuda:
        return loss_variant_deep_supervision_loss_eager(outputs, targets, variant, batch_dice, ddp, ignore_label)
    if variant == "dice_ce_nosmooth":
        return deep_supervision_loss(outputs, targets, batch_dice, ddp, smooth, ignore_label)
    from . import ops
    w_ce, w = _level_constants(tuple(o.numel() // o.shape[1] for o in outputs), outputs[0].device)
    if kpercent is not None:
        ip, gt, rec = ops.topk_ce_stats(list(outputs), list(targets), ignore_label, eps, kpercent, with_dice)
        total = (w * rec[:, 3]).sum()                                           # (L,) TopKLoss per level
        return total + (w * _dice_levels(ip, gt, batch_dice, ddp, smooth)).sum() if with_dice else total
    if variant == "dice":
        ip, gt, _ = ops.dice_ce_stats(list(outputs), list(targets), None)
        return (w * _dice_levels(ip, gt, batch_dice, ddp, smooth)).sum()
    _, gt, ce = ops.dice_ce_stats(list(outputs), list(targets), ignore_label)     # "ce"
    if ignore_label is not None:
        w_ce = w / gt.sum((1, 2)).clamp(min=1.0)                                # the mean over the valid pixels, as in deep_supervision_loss
    return (w_ce * ce).sum()


# ------------------------------------------------------------------------------------------------
# loss of region-based datasets (sigmoid heads)
# ------------------------------------------------------------------------------------------------
def regions_from_label_map(target, regions, ignore_label=None):
    """A label map (B, 1, ...) as the float region planes (B, R, ...) that nnU-Net's ConvertSegmentationToRegionsTransform writes --
    plane r is ``np.isin(seg, regions[r])`` -- followed, with an ignore label, by the plane of the pixels that carry it."""
    planes = []
    for r in regions:
        values = torch.as_tensor([int(v) for v in (r if isinstance(r, (tuple, list)) else (r,))], device=target.device).to(target.dtype)
        planes.append(torch.isin(target, values))
    if ignore_label is not None:
        planes.append(target == ignore_label)
    return torch.cat(planes, 1).to(target.dtype)


def dc_and_bce_loss(logits, target, batch_dice=True, ddp=False, use_ignore_label=False, smooth=1e-5, weight_ce=1.0, weight_dice=1.0):
    """DC_and_BCE_loss.forward (loss/compound_losses.py:84-100) as nnUNetTrainer.py:330-336 builds it, in torch ops, one level:
    MemoryEfficientSoftDiceLoss(apply_nonlin=sigmoid, do_bg=True, smooth=1e-5) + BCEWithLogitsLoss.  target: region planes
    (B, R, ...); with use_ignore_label the ignore plane follows them (B, R + 1, ...) and masks both terms.  weight_ce / weight_dice:
    the weights of DC_and_BCE_loss; (0, 1) is the Dice term alone, the loss of nnUNetTrainerDiceLoss for regions."""
    axes = tuple(range(2, logits.ndim))
    probs = torch.sigmoid(logits)
    if use_ignore_label:
        mask = (1 - target[:, -1:]).bool()
        target = target[:, :-1]
        with torch.no_grad():
            sum_gt = (target * mask).sum(axes)
        intersect = (probs * target * mask).sum(axes)
        sum_pred = (probs * mask).sum(axes)
    else:
        mask = None
        with torch.no_grad():
            sum_gt = target.sum(axes)
        intersect = (probs * target).sum(axes)
        sum_pred = probs.sum(axes)
    if batch_dice:
        stats = torch.stack([intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)])
        if ddp:
            stats = _AllGatherSum.apply(stats)
        intersect, sum_pred, sum_gt = stats[0], stats[1], stats[2]
    dc = -((2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)).mean()
    if weight_ce == 0:
        return weight_dice * dc
    if mask is None:
        bce = F.binary_cross_entropy_with_logits(logits, target)
    else:
        bce = (F.binary_cross_entropy_with_logits(logits, target, reduction="none") * mask).sum() / torch.clip(mask.sum(), min=1e-8)
    return bce + dc if weight_ce == 1 and weight_dice == 1 else weight_ce * bce + weight_dice * dc


def region_deep_supervision_loss_eager(outputs, targets, regions=None, batch_dice=True, ddp=False, smooth=1e-5, ignore_label=None,
                                       weight_ce=1.0, weight_dice=1.0):
    """The region loss as the reference composes it, level by level in torch ops (host tensors, CPU tests, more than 16 heads)."""
    if regions is not None:
        targets = [regions_from_label_map(t, regions, ignore_label) for t in targets]
    ws = deep_supervision_weights(len(outputs))
    total = None
    for w, o, t in zip(ws, outputs, targets):
        level = w * dc_and_bce_loss(o, t, batch_dice, ddp, ignore_label is not None, smooth, weight_ce, weight_dice)
        total = level if total is None else total + level
    return total


def region_deep_supervision_loss(outputs, targets, regions=None, batch_dice=True, ddp=False, smooth=1e-5, ignore_label=None,
                                 weight_ce=1.0, weight_dice=1.0):
    """DeepSupervisionWrapper(DC_and_BCE_loss) of reference nnUNetTrainer.py:330-352, the loss of region-based datasets.
    regions: the label manager's ``foreground_regions`` -- the targets are then LABEL MAPS (B, 1, ...) and ``ignore_label`` is the label
    value that masks a pixel; None: the targets are REGION PLANES (B, R, ...) as ConvertSegmentationToRegionsTransform delivers them,
    and ``ignore_label is not None`` says that the ignore plane follows them (B, R + 1, ...).
    On the MI355X: K29 reads every logit map once for the statistics and once for the gradient; the (levels, heads)-sized algebra
    below is torch, vectorised over the levels, and the batch-dice statistics of all levels cross the ranks in ONE all-reduce each way.
    Dice keeps all R heads (do_bg=True).  Without an ignore label the cross-entropy is the mean over B R HW elements; with one it is
    the masked sum over clip(mask sum, 1e-8) -- the mask sum has no factor R and is local to the rank (compound_losses.py:96) -- so a
    fully ignored level gives 0 there and -1 from the dice.  CPU tensors, and more than 16 heads, take the eager composition.
    weight_ce / weight_dice: the weights of DC_and_BCE_loss (1 / 1 as the trainer builds it; 0 / 1 with smooth 1e-5 is the Dice-only
    loss of nnUNetTrainerDiceLoss, 1 / 1 with smooth 0 the loss of nnUNetTrainerDiceCELoss_noSmooth)."""
    from . import ops
    if not outputs[0].is_cuda or outputs[0].shape[1] > ops.REGION_LOSS_MAX_REGIONS:
        return region_deep_supervision_loss_eager(outputs, targets, regions, batch_dice, ddp, smooth, ignore_label, weight_ce, weight_dice)
    member = None if regions is None else ops.region_member_table(regions, outputs[0].device)
    ip, gt, sums = ops.dice_bce_stats(list(outputs), list(targets), member, ignore_label)     # (L, B, 2, R), (L, B, R), (L, 2)
    inter, pred = ip[:, :, 0], ip[:, :, 1]
    if batch_dice:
        stats = torch.stack([inter.sum(1), pred.sum(1), gt.sum(1)])             # (3, L, R)
        if ddp:
            stats = _AllGatherSum.apply(stats)
        inter, pred, gt = stats[0], stats[1], stats[2]
    dc = (2 * inter + smooth) / torch.clip(gt + pred + smooth, 1e-8)
    dice = -dc.flatten(1).mean(1)                                               # (L,)
    w_bce, w_dice = _level_constants(tuple(o.numel() for o in outputs), sums.device)      # BCE mean over B * R * HW elements
    if ignore_label is not None:
        w_bce = w_dice / sums[:, 1].clamp(min=1e-8)
    if weight_ce == 1 and weight_dice == 1:
        return (w_bce * sums[:, 0] + w_dice * dice).sum()
    if weight_ce == 0:
        return weight_dice * (w_dice * dice).sum()
    return (weight_ce * (w_bce * sums[:, 0]) + weight_dice * (w_dice * dice)).sum()


# ------------------------------------------------------------------------------------------------
# optimiser / schedule
# ------------------------------------------------------------------------------------------------
class ClipOptimizer(torch.optim.Optimizer):
    """What the fused clip + update optimizers share (K11: ``ClipAdamW``; K34: ``ClipSGD``, ``ClipAdam``): the pointer table and the work
    list of the kernels, the pinned upload of the gradient addresses, the device-resident learning rate and step counter of the
    capturable form with its one capture per optimizer, and a ``load_state_dict`` that keeps the state tensors in place.
    A subclass names its per-parameter state tensors in ``_STATE`` (in the order of the table: two columns, a third goes into the extra
    pointer block), says in ``_HAS_STEP`` whether torch's state carries a ``step`` entry, names its kernel's kind constant of the header
    (``MLAGG_OPT_*``) in ``_KIND`` and gives the group's hyper-parameters in ``_hyper``."""
    _STATE = ()
    _HAS_STEP = True
    _KIND = None

    def __init__(self, params, defaults, capturable=False):
        params = list(params)
        super().__init__(params, defaults)
        self._name = type(self).__name__
        if len(self.param_groups) != 1:
            # the clip norm is the norm over ALL parameters (clip_grad_norm_(network.parameters(), 12), B:855): one group
            raise RuntimeError(f"{self._name}: one parameter group (the reference passes network.parameters(), T:138)")
        self.capturable = bool(capturable)
        # hipGraph form (GraphedTrainStep): the step counter and a COPY of the learning rate live on the device.  ``param_groups``
        # keeps the learning rate as the Python float that schedules assign and training loops log, round and pickle; ``sync_lr``
        # carries it to the device copy before a replay
        lr = float(self.param_groups[0]["lr"])
        self._step_dev = torch.zeros(1, dtype=torch.int32, device=params[0].device) if capturable else None
        self._lr_dev = torch.full((1,), lr, dtype=torch.float32, device=params[0].device) if capturable else None
        self._steps = 0
        self._work = {}
        self._tables = {}                             # capturable: per (parameter set, captured?) (pinned host table, device table)
        self._sumsq = None
        self._stepped = None                          # ids of the parameters of the first step

    def _state_of(self, p):
        st = self.state[p]
        if not st:
            if self._HAS_STEP:
                st["step"] = torch.tensor(0.0)
            for k in self._STATE:
                st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _upload_len(self, T):
        """int64 entries of the upload buffer of T parameter tensors: the rows, and one more pointer each with a third state tensor."""
        return (6 if len(self._STATE) > 2 else 5) * T

    def _rows_and_third(self, buf, T):
        """The two named parts of a flat upload buffer (host or device), as views of it: the (T, 5) rows (param, grad, state 0,
        state 1, numel) the kernels index, and behind them the T pointers to the third state tensor (None for two or fewer).
        5 T int64 entries keep the second part 8-byte aligned."""
        return buf[:5 * T].view(T, 5), (buf[5 * T:] if len(self._STATE) > 2 else None)

    def steps_done(self):
        """Optimisation steps so far (capturable: read from the device counter the replays advance; that synchronises)."""
        return int(self._step_dev.item()) if self.capturable else self._steps

    def state_dict(self):
        if self._HAS_STEP:
            n = float(self.steps_done())
            for st in self.state.values():
                if st:
                    st["step"] = torch.tensor(n)
        return super().state_dict()

    def sync_lr(self):
        """Capturable form: write ``param_groups[0]["lr"]`` into the device copy that the update kernel -- and a captured graph --
        reads.  ``GraphedTrainStep`` calls this before every replay and an eager ``step`` calls it itself; whoever replays a graph
        of their own calls it after changing the learning rate.  Never inside a capture: the fill would be recorded with the
        value of that moment and every replay would write it back."""
        if self.capturable:
            self._lr_dev.fill_(float(self.param_groups[0]["lr"]))

    def _check_loaded_group(self, group):
        """Refuse a loaded parameter group that asks for arithmetic the kernels do not implement."""

    def load_state_dict(self, sd):
        # capturable: a captured graph holds the ADDRESSES of the state tensors, of the work list and of its pointer table, so
        # the loaded state is copied into the existing tensors and all of these stay in place
        keep = {p: tuple(st[k] for k in self._STATE) for p, st in self.state.items() if st} if self.capturable else {}
        for g in sd["param_groups"]:
            self._check_loaded_group(g)               # before anything of this optimizer changes
        super().load_state_dict(sd)
        for g in self.param_groups:
            g["lr"] = float(g["lr"])                  # a checkpoint written while the learning rate was a device tensor
        for p, st in self.state.items():
            for k in self._STATE:
                if st and st.get(k, 0) is None:       # torch.optim.SGD writes ``momentum_buffer: None`` until a buffer exists
                    st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif st and k not in st:
                    raise RuntimeError(f"{self._name}: the checkpoint holds no {k!r} for a parameter")
        for p, kept in keep.items():
            st = self.state[p]
            for k, t in zip(self._STATE, kept):
                if st:
                    t.copy_(st[k])
                else:                                 # a checkpoint from before the first step
                    t.zero_()
            if not st and self._HAS_STEP:
                st["step"] = torch.tensor(0.0)
            for k, t in zip(self._STATE, kept):
                st[k] = t
        if not self.capturable:
            self._work.clear()                        # the state tensors were replaced: cached addresses are stale
        self._stepped = None
        if self._HAS_STEP:
            steps = [int(st["step"]) for st in self.state.values() if st and "step" in st]
            self._steps = max(steps) if steps else 0
            if self.capturable:
                self._step_dev.fill_(self._steps)

    def _hyper(self, group):
        """(beta1 or momentum, beta2, eps) of the group as the kernel takes them."""
        raise NotImplementedError

    def _launch(self, group, table, extra, work, max_norm, device_form, scaler=None):
        """Launch the kernels of one step: ``table`` / ``extra`` / ``work`` are device tensors (``extra`` None without a third state
        tensor); ``device_form``: read the learning rate and the step from ``_lr_dev`` / ``_step_dev``, else ``group["lr"]`` and
        ``_steps`` as launch arguments.  ``scaler``: the loss-scaled step (K35) of ``DeviceGradScaler.step``, the device form alone,
        with the scaler's device state."""
        from . import _lib
        b1, b2, eps = self._hyper(group)
        head = (_lib.CONSTANTS[self._KIND], table.data_ptr(), extra.data_ptr() if extra is not None else None, work.data_ptr(),
                work.shape[0], self._sumsq.data_ptr())
        tail = (b1, b2, eps, float(group["weight_decay"]), max_norm)
        if scaler is not None:
            _lib.launch("mlagg_scaled_clip_step_dev", *head, self._lr_dev.data_ptr(), self._step_dev.data_ptr(), scaler._scale.data_ptr(),
                        scaler._growth_tracker.data_ptr(), scaler.found_inf.data_ptr(), scaler._mult.data_ptr(), *tail,
                        scaler.growth_factor, scaler.backoff_factor, scaler.growth_interval)
        elif device_form:
            _lib.launch("mlagg_optimizer_clip_step_dev", *head, self._lr_dev.data_ptr(), self._step_dev.data_ptr(), *tail)
        else:
            _lib.launch("mlagg_optimizer_clip_step", *head, float(group["lr"]), *tail, self._steps)

    @torch.no_grad()
    def step(self, closure=None, max_norm=0.0, _grad_scaler=None):
        """``_grad_scaler`` is private to ``DeviceGradScaler.step``, which passes itself: the loss-scaled step of K35 on gradients that
        carry its scale, capturable form only.  The scaler checks the device and keeps the one-optimizer-per-iteration bookkeeping;
        nobody else passes the argument."""
        from . import _lib
        grad_scaler = _grad_scaler
        if grad_scaler is not None and not self.capturable:
            raise RuntimeError(f"{type(self).__name__}: DeviceGradScaler needs capturable=True (a skipped step can be left uncounted "
                               "without a host synchronisation only in the device-resident step counter)")
        chunk = _lib.lib().mlagg_adamw_chunk_elements()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if grad_scaler is None:
            self._steps += 1                          # (the scaled step counts on the device, and only the applied steps)
        from . import ops
        ops.invalidate_weight_images()                # the kernels below rewrite the parameters through raw pointers: no version bump
        name = self._name
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            dev = ps[0].device
            key = tuple(id(p) for p in ps)
            # ONE step counter serves every parameter (bias correction is a launch argument): right as long as the same
            # parameters receive a gradient every step, which holds on this path; a changing set would silently give the
            # late-comers torch.optim.AdamW's step-1 correction at step k, so it is refused
            if self._stepped is None:
                self._stepped = key
            elif key != self._stepped:
                raise RuntimeError(f"{name}: the set of parameters with a gradient changed between steps")
            T = len(ps)
            if key not in self._work:
                # per parameter set: the work list and the static columns of the pointer table (uploaded once).  Rows of
                # (param, grad, state 0, state 1, numel); behind the T rows one pointer per row for a third state tensor
                for p in ps:
                    self._state_of(p)
                    if not (p.is_cuda and p.is_contiguous() and p.dtype == torch.float32):
                        raise RuntimeError(f"{name}: fp32 contiguous parameters on the MI355X expected")
                numels = [p.numel() for p in ps]
                wl = [(i, c) for i, n in enumerate(numels) for c in range((n + chunk - 1) // chunk)]
                # ONE flat upload buffer: 5 T entries of rows, then (three state tensors only) T pointers to the third
                base = torch.zeros(self._upload_len(T), dtype=torch.int64)
                rows, third = self._rows_and_third(base, T)
                rows[:, 0] = torch.tensor([p.data_ptr() for p in ps], dtype=torch.int64)
                rows[:, 4] = torch.tensor(numels, dtype=torch.int64)
                for i, k in enumerate(self._STATE):
                    ptrs = torch.tensor([self.state[p][k].data_ptr() for p in ps], dtype=torch.int64)
                    if i < 2:
                        rows[:, 2 + i] = ptrs
                    else:
                        third.copy_(ptrs)
                self._work[key] = (torch.tensor(wl, dtype=torch.int32).to(dev), base)
            work, base = self._work[key]
            # only the gradient addresses change from step to step (zero_grad(set_to_none=True)); the table goes up through
            # pinned memory without blocking the host (a pageable copy would make the CPU wait for the GPU every step)
            host = base.clone()
            self._rows_and_third(host, T)[0][:, 1] = torch.tensor([p.grad.data_ptr() for p in ps], dtype=torch.int64)
            for p in ps:
                if not (p.grad.is_contiguous() and p.grad.dtype == torch.float32):
                    raise RuntimeError(f"{name}: fp32 contiguous gradients expected")
            if self._sumsq is None or self._sumsq.device != dev or self._sumsq.numel() != 1 + work.shape[0]:
                self._sumsq = torch.zeros(1 + work.shape[0], dtype=torch.float64, device=dev)       # [0]: total; one partial per work item
            if self.capturable:
                # a table that OUTLIVES the call (a replayed graph reads it): one pinned host copy + one device copy per parameter
                # set, re-uploaded only when a gradient address changed.  Inside a capture the upload becomes a copy node out of
                # the pinned buffer, whose content then no longer changes (captured gradients sit at fixed addresses): captured
                # steps have a pair of their own, which no eager step -- with its own gradient addresses -- ever writes.  Both
                # pairs are allocated at the first step, whichever form it is: a capture that follows an eager or warm-up step then
                # pins no memory (a first step INSIDE a capture still does, as it always did), at the price of one unused pair
                # (40 bytes per parameter tensor, 48 with a third state tensor) in an optimizer that is never captured
                capturing = torch.cuda.is_current_stream_capturing()
                for c in (False, True):
                    if (key, c) not in self._tables:
                        self._tables[key, c] = (torch.full_like(host, -1).pin_memory(), torch.empty_like(host, device=dev))
                pinned, table = self._tables[key, capturing]
                if not torch.equal(pinned, host):
                    if not capturing:
                        torch.cuda.current_stream().synchronize()      # an earlier upload may still be reading the pinned buffer
                    elif int(pinned.reshape(-1)[0]) != -1:     # the first entry is a parameter address; -1 is the fill of a table never written
                        raise RuntimeError(f"{name}: a second capture with other gradient addresses would redirect the first "
                                           "graph's update; one captured step per optimizer")
                    pinned.copy_(host)
                    table.copy_(pinned, non_blocking=True)
                if not capturing:
                    self.sync_lr()
                self._launch(group, *self._rows_and_third(table, T), work, float(max_norm), True, grad_scaler)
                continue
            table = host.pin_memory().to(dev, non_blocking=True)
            self._launch(group, *self._rows_and_third(table, T), work, float(max_norm), False)
            self._keepalive = table                   # the table must outlive the asynchronous launches
        return loss

    def grad_norm(self):
        """||g||_2 of the last step (device tensor; reading it synchronises)."""
        return self._sumsq[:1].sqrt().float()


class ClipAdamW(ClipOptimizer):
    """clip_grad_norm_(max_norm) + AdamW in two launches for all parameters (K11).  Same hyper-parameters, arithmetic and
    ``state_dict`` layout (per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``) as ``torch.optim.AdamW``; the clip
    coefficient is computed on the device (no host synchronisation) and the gradients in memory stay unscaled."""
    _STATE = ("exp_avg", "exp_avg_sq")
    _KIND = "MLAGG_OPT_ADAMW"

    def __init__(self, params, lr=5e-4, betas=(0.9, 0.999), eps=1e-4, weight_decay=3e-5, capturable=False):
        super().__init__(params, dict(lr=float(lr), betas=betas, eps=eps, weight_decay=weight_decay), capturable)

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return float(b1), float(b2), float(group["eps"])


class ClipSGD(ClipOptimizer):
    """clip_grad_norm_(max_norm) + torch.optim.SGD(momentum, nesterov=True) -- the optimizer of the reference's base trainer
    (nnUNetTrainer.py:448-452: lr 1e-2, momentum 0.99, weight decay 3e-5) -- in two launches for all parameters (K34).  Hyper-parameters,
    arithmetic (dampening 0; a zero buffer gives torch's first step) and ``state_dict`` layout (per parameter ``momentum_buffer``; the
    group keys torch writes) are torch.optim.SGD's: a checkpoint of either loads into the other.  ``capturable=True`` keeps a copy of
    the learning rate on the device, so a step captured into a hipGraph follows the schedule -- what torch.optim.SGD, whose learning
    rate is baked into the captured launches, cannot do.  torch's SGD state carries no step count: ``steps_done`` counts the steps of
    this object and ``load_state_dict`` leaves it alone."""
    _STATE = ("momentum_buffer",)
    _HAS_STEP = False
    _KIND = "MLAGG_OPT_SGD_NESTEROV"

    def __init__(self, params, lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=True, capturable=False, *, dampening=0):
        defaults = dict(lr=float(lr), momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        self._check_loaded_group(defaults)
        super().__init__(params, defaults, capturable)

    def _check_loaded_group(self, group):
        if not group["nesterov"]:
            raise RuntimeError("ClipSGD: nesterov=False is not implemented (the kernel computes p -= lr (g + momentum buf), the "
                               "Nesterov step of the reference's trainers)")
        if group["dampening"] != 0:
            raise RuntimeError("ClipSGD: dampening must be 0 (torch.optim.SGD itself refuses Nesterov momentum with dampening, "
                               "and the kernel computes buf = momentum buf + g)")
        if not group["momentum"] > 0:
            raise RuntimeError("ClipSGD: Nesterov momentum needs momentum > 0, as torch.optim.SGD says")
        if group.get("maximize"):
            raise RuntimeError("ClipSGD: maximize is not implemented")

    def _hyper(self, group):
        return float(group["momentum"]), 0.0, 0.0


class ClipAdam(ClipOptimizer):
    """clip_grad_norm_(max_norm) + Adam in two launches for all parameters (K34), in the two forms the reference's optimizer-variant
    trainers use (variants/optimizer/nnUNetTrainerAdam.py): ``amsgrad=True, decoupled=True`` is nnUNetTrainerAdam's
    torch.optim.AdamW(amsgrad=True), ``amsgrad=False, decoupled=False`` nnUNetTrainerVanillaAdam's torch.optim.Adam with L2 weight
    decay.  State keys and group keys are torch's (``step``, ``exp_avg``, ``exp_avg_sq`` and, with amsgrad, ``max_exp_avg_sq``), so
    checkpoints go both ways.  The other two combinations have no kernel and are refused (amsgrad off with decoupled decay is
    ``ClipAdamW``)."""
    _KINDS = {(True, True): "MLAGG_OPT_ADAMW_AMSGRAD", (False, False): "MLAGG_OPT_ADAM_L2"}

    def __init__(self, params, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=3e-5, amsgrad=True, decoupled=True, capturable=False):
        defaults = dict(lr=float(lr), betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad), maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled))
        self._check_loaded_group(defaults)
        self._KIND = self._KINDS[bool(amsgrad), bool(decoupled)]
        self._STATE = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq") if amsgrad else ("exp_avg", "exp_avg_sq")
        super().__init__(params, defaults, capturable)

    def _check_loaded_group(self, group):
        # a torch.optim.Adam / AdamW from before the key existed: the recipe this optimizer was built for
        decoupled = group["decoupled_weight_decay"] if "decoupled_weight_decay" in group else self.defaults["decoupled_weight_decay"]
        form = (bool(group["amsgrad"]), bool(decoupled))
        if form not in self._KINDS:
            raise RuntimeError(f"ClipAdam: amsgrad={form[0]}, decoupled={form[1]} has no kernel; the reference's recipes are "
                               "amsgrad=True, decoupled=True (AdamW with amsgrad) and amsgrad=False, decoupled=False (Adam with L2 "
                               "decay); AdamW without amsgrad is ClipAdamW")
        if getattr(self, "_KIND", None) is not None and self._KINDS[form] != self._KIND:
            raise RuntimeError(f"ClipAdam: the checkpoint was written with amsgrad={form[0]}, decoupled={form[1]}, this optimizer "
                               "was built for the other recipe")
        if group.get("maximize"):
            raise RuntimeError("ClipAdam: maximize is not implemented")

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return float(b1), float(b2), float(group["eps"])


class DeviceGradScaler:
    """``torch.amp.GradScaler`` of the reference's fp16 step (nnUNetTrainer.py:152, :848-858) with its decisions on the device (K35):
    the scale, the growth tracker and ``found_inf`` are device tensors, and ``step`` with a capturable ``ClipOptimizer`` is that
    optimizer's three launches -- the norm of the unscaled gradients, the overflow test, the skipped or applied step, the new scale --
    with no host synchronisation (``GradScaler.step`` reads ``found_inf.item()``), no rewrite of the gradients (``unscale_``; they stay
    scaled and unclipped in memory) and nothing a hipGraph capture cannot record.  One deviation from torch: finite gradients whose
    unscaled square -- or a 64 Ki-element chunk's fp32 sum of squares -- leaves fp32 (|g / scale| or the chunk norm > 1.8e19) count as an overflow and skip the step; torch would step with a zero coefficient.

    ``step`` does the update of the scale as well; ``update`` is kept for the reference's call shape and closes the iteration: one
    optimizer per iteration.  With a ``ClipOptimizer`` it requires ``capturable=True``: the device step counter is the only place a
    skipped step can be left uncounted without a synchronisation, and ``steps_done()`` then counts the applied steps.  A plain torch
    optimizer (the one ``configure_optimizers`` gives host parameters) takes the same decisions through torch ops (unscale, norm, skip,
    ``torch._amp_update_scale_``), with torch's synchronisation; a ``ClipOptimizer`` over host parameters is refused, its kernels
    have no host form.  ``state_dict`` / ``load_state_dict`` carry ``torch.amp.GradScaler``'s keys, so a checkpoint's
    ``grad_scaler_state`` loads into either class; loading writes into the existing device tensors (a captured graph holds their
    addresses)."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not growth_factor > 1.0:
            raise RuntimeError("DeviceGradScaler: growth_factor must be > 1")
        if not 0.0 < backoff_factor < 1.0:
            raise RuntimeError("DeviceGradScaler: backoff_factor must be in (0, 1)")
        if int(growth_interval) < 1:
            raise RuntimeError("DeviceGradScaler: growth_interval must be at least 1")
        self.device = torch.device(device)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self._scale = torch.full((1,), float(init_scale), dtype=torch.float32, device=self.device)
        self._growth_tracker = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.found_inf = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._mult = torch.zeros(1, dtype=torch.float32, device=self.device)      # scratch: (1 / scale) * clip coefficient
        self._open = False                                                         # a step since the last update()

    def scale(self, loss):
        return loss * self._scale.reshape(())

    def get_scale(self):
        """The scale as a Python float (synchronises)."""
        return float(self._scale.item())

    def get_growth_tracker(self):
        return int(self._growth_tracker.item())

    def is_enabled(self):
        return True

    @torch.no_grad()
    def step(self, optimizer, max_norm=0.0):
        """Unscale, clip to ``max_norm`` (<= 0: no clipping), step unless a gradient overflowed, update the scale."""
        if self._open:
            raise RuntimeError("DeviceGradScaler: one optimizer per iteration (step() already ran since the last update())")
        params = [p for g in optimizer.param_groups for p in g["params"] if p.grad is not None]
        if isinstance(optimizer, ClipOptimizer):
            if not all(p.is_cuda for p in params):
                raise RuntimeError(f"DeviceGradScaler: {type(optimizer).__name__} has no host form; host parameters take the torch "
                                   "optimizer of the recipe (configure_optimizers returns it for a host model)")
            if not optimizer.capturable:
                raise RuntimeError(f"DeviceGradScaler: {type(optimizer).__name__} must be built with capturable=True (the device step "
                                   "counter is the only place a skipped step can be left uncounted without a synchronisation)")
            if any(p.device != self._scale.device for p in params):
                raise RuntimeError("DeviceGradScaler: the parameters live on another device than the scale")
            optimizer.step(max_norm=max_norm, _grad_scaler=self)
            self._open = True
            return None
        # a plain torch optimizer (host or device parameters): the same decisions through torch ops, as torch orders them
        inv = self._scale.double().reciprocal().float()
        total = torch.zeros((), dtype=torch.float64, device=self._scale.device)
        for p in params:
            p.grad.mul_(inv.to(p.grad.device).reshape(()))                         # unscale_: rewrites the gradients
            total += p.grad.float().pow(2).sum().double().to(total.device)
        bad = not bool(torch.isfinite(total))                                      # synchronises, as GradScaler.step does
        self.found_inf.fill_(1.0 if bad else 0.0)
        out = None
        if not bad:
            if max_norm > 0:
                coef = torch.clamp(max_norm / (total.sqrt().float() + 1e-6), max=1.0)
                for p in params:
                    p.grad.mul_(coef.to(p.grad.device))
            out = optimizer.step()
        torch._amp_update_scale_(self._scale, self._growth_tracker, self.found_inf, self.growth_factor, self.backoff_factor,
                                 self.growth_interval)
        self._open = True
        return out

    def update(self):
        """Closes the iteration; the scale was updated by ``step`` already (on the device, behind the overflow test)."""
        self._open = False

    def state_dict(self):
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self.get_growth_tracker()}

    def load_state_dict(self, state_dict):
        """The scale and the tracker go into the existing device tensors.  The two factors and the interval are launch arguments: a
        step captured before the load keeps the ones it was captured with."""
        if len(state_dict) == 0:
            raise RuntimeError("DeviceGradScaler: the source state dict is empty, possibly because it was saved from a disabled GradScaler")
        self._scale.fill_(float(state_dict["scale"]))                              # in place: a captured graph holds the addresses
        self._growth_tracker.fill_(int(state_dict["_growth_tracker"]))
        self.growth_factor, self.backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self.growth_interval = int(state_dict["growth_interval"])


OPTIMIZERS = ("adamw", "sgd", "adam", "vanilla_adam")


def configure_optimizers(model, initial_lr=None, weight_decay=3e-5, fused=None, capturable=False, optimizer="adamw", num_epochs=1000):
    """optimizer "adamw" (the default): AdamW + cosine schedule of reference T:137-147, initial_lr 5e-4.  The reference's other recipes,
    initial_lr 1e-2 and PolyLR over ``num_epochs`` (nnUNetTrainer.py:146-149):
      "sgd"           the base trainer's SGD(momentum 0.99, nesterov) (nnUNetTrainer.py:448-452)                 ClipSGD (K34)
      "adam"          nnUNetTrainerAdam's AdamW(amsgrad=True) (variants/optimizer/nnUNetTrainerAdam.py:9-18)    ClipAdam (K34)
      "vanilla_adam"  nnUNetTrainerVanillaAdam's Adam with L2 decay (:21-30)                                    ClipAdam (K34)
    ``capturable=True`` keeps the step counter and a copy of the learning rate on the device so that the whole step can live inside
    one hipGraph (GraphedTrainStep).  Host parameters get the torch optimizer of the same recipe."""
    if optimizer not in OPTIMIZERS:
        raise RuntimeError(f"optimizer {optimizer!r}: one of {OPTIMIZERS}")
    # every parameter, in module order, as the reference's ``AdamW(self.network.parameters(), ...)`` (T:138): the
    # frozen ``dummy_tensor`` keeps its slot, so parameter indices in optimizer checkpoints equal the reference's
    params = list(model.parameters())
    if fused is None:
        fused = all(p.is_cuda for p in params)
    on_device = fused and all(p.is_cuda for p in params)
    if optimizer != "adamw":
        lr = 1e-2 if initial_lr is None else initial_lr
        if optimizer == "sgd":
            opt = ClipSGD(params, lr, 0.99, weight_decay, capturable=capturable) if on_device else \
                torch.optim.SGD(params, lr, weight_decay=weight_decay, momentum=0.99, nesterov=True)
        elif optimizer == "adam":
            opt = ClipAdam(params, lr, weight_decay=weight_decay, amsgrad=True, decoupled=True, capturable=capturable) if on_device else \
                torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, amsgrad=True)
        else:
            opt = ClipAdam(params, lr, weight_decay=weight_decay, amsgrad=False, decoupled=False, capturable=capturable) if on_device else \
                torch.optim.Adam(params, lr=lr, weight_decay=weight_decay)
        return opt, PolyLRSchedule(opt, lr, num_epochs)
    initial_lr = 5e-4 if initial_lr is None else initial_lr
    if on_device:
        # on the device: clip + AdamW of all parameters in three launches (K11); capturable: lr and step counter device-resident
        opt = ClipAdamW(params, initial_lr, weight_decay=weight_decay, eps=1e-4, capturable=capturable)
        return opt, CosineLRSchedule(opt, t_initial=500, lr_min=1e-6, warmup_t=10, warmup_lr_init=1e-4)
    lr = torch.tensor(initial_lr, device=params[0].device, dtype=torch.float32) if capturable else initial_lr
    opt = torch.optim.AdamW(params, lr, weight_decay=weight_decay, eps=1e-4, fused=fused, capturable=capturable)
    return opt, CosineLRSchedule(opt, t_initial=500, lr_min=1e-6, warmup_t=10, warmup_lr_init=1e-4)


class PolyLRSchedule:
    """PolyLRScheduler of the reference (training/lr_scheduler/polylr.py): lr = initial_lr (1 - step / max_steps) ** exponent, stepped
    with the epoch index at epoch start (nnUNetTrainer.py:825).  ``step()`` without an epoch -- or with -1 -- takes an internal counter
    and advances it; as in the reference, whose base class steps once on construction, the constructor takes the counter's step 0.  The
    learning rate is assigned as a float in ``param_groups`` (``ClipOptimizer.sync_lr`` carries it to a captured graph)."""

    def __init__(self, optimizer, initial_lr, max_steps, exponent=0.9):
        self.optimizer, self.initial_lr, self.max_steps, self.exponent = optimizer, initial_lr, max_steps, exponent
        self.ctr = 0
        self.step()

    def lr_at(self, current_step):
        return self.initial_lr * (1 - current_step / self.max_steps) ** self.exponent

    def step(self, current_step=None):
        if current_step is None or current_step == -1:
            current_step = self.ctr
            self.ctr += 1
        for g in self.optimizer.param_groups:
            g["lr"] = self.lr_at(current_step)


class CosineLRSchedule:
    """timm CosineLRScheduler semantics for one cycle, stepped with the epoch index at epoch start
    (reference nnUNetTrainer.py:825)."""

    def __init__(self, optimizer, t_initial, lr_min, warmup_t, warmup_lr_init):
        self.opt, self.t_initial, self.lr_min = optimizer, t_initial, lr_min
        self.warmup_t, self.warmup_lr_init = warmup_t, warmup_lr_init
        self.base = [float(g["lr"]) for g in optimizer.param_groups]

    def lr_at(self, epoch, base):
        if epoch < self.warmup_t:
            return self.warmup_lr_init + epoch * (base - self.warmup_lr_init) / self.warmup_t
        if epoch >= self.t_initial:
            return self.lr_min
        return self.lr_min + 0.5 * (base - self.lr_min) * (1 + math.cos(math.pi * epoch / self.t_initial))

    def step(self, epoch):
        for g, base in zip(self.opt.param_groups, self.base):
            if torch.is_tensor(g["lr"]):
                g["lr"].fill_(self.lr_at(epoch, base))      # torch's own capturable optimizers keep a tensor there
            else:
                g["lr"] = self.lr_at(epoch, base)           # ClipAdamW: a float in both forms (ClipAdamW.sync_lr)


# ------------------------------------------------------------------------------------------------
# data parallelism
# ------------------------------------------------------------------------------------------------
def split_batch_size(global_batch, world_size):
    """Per-rank batch sizes that always sum to ``global_batch`` and are never zero or negative
    (the reference's ceil-based split yields (2,2,2,2,2,0,-2,-4) for 10 over 8, SURVEY finding 7c)."""
    if global_batch < world_size:
        raise RuntimeError("Cannot run DDP if the batch size is smaller than the number of GPUs")
    base, rem = divmod(global_batch, world_size)
    return [base + (1 if r < rem else 0) for r in range(world_size)]


class BucketedGradSync:
    """Data-parallel gradient exchange for device parameters without DistributedDataParallel's per-parameter kernels.

    torch's DDP copies every gradient into its bucket with its own kernel (and scales it there): 456 launches of ~4 us per step for
    the 524 gradients of this network (profiles/round3_j_ddp_single_rank_trace.md: 1.8 ms of a 38 ms step, before a single byte is
    exchanged).  Here the parameters are cut into buckets in reverse registration order for the FIRST step, and from the second step
    on in the order that step's backward actually delivered the gradients (what DDP's bucket rebuild does: registration order has
    ``downs.i`` behind all ``layers.j``, backward interleaves them, and the round-4 trace showed five of ten buckets -- half of the
    108 MB -- becoming complete at 95 % of backward: profiles/round4_f_ddp_bucket_timeline_registration_order.md); a small first bucket so that the
    exchange starts early; when the last gradient of a bucket has been accumulated
    (``register_post_accumulate_grad_hook``) the bucket's gradients are gathered into its flat buffer by ONE multi-tensor copy,
    scaled by 1 / world once, and all-reduced asynchronously (RCCL on its own stream, overlapped with the rest of backward).
    ``finish()`` -- called by ``train_step`` after backward -- waits for the exchanges and points every ``p.grad`` at its slice of
    the averaged buffer (no scatter copy: the optimizer reads the gradients where the collective left them)."""

    def __init__(self, module, bucket_cap_mb=25, first_bucket_mb=1, group=None, last_bucket_mb=2):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group)
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise RuntimeError("BucketedGradSync: no trainable parameters")
        if any(p.dtype != torch.float32 for p in params) or len({p.device for p in params}) != 1:
            raise RuntimeError("BucketedGradSync: fp32 parameters on one device expected")
        # replicas start from rank 0's parameters (what DDP's constructor does), in one coalesced broadcast
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1) for p in params])
            dist.broadcast(flat, 0, group=group)
            off = 0
            for p in params:
                p.copy_(flat[off:off + p.numel()].view_as(p))
                off += p.numel()
        self._caps = (int(first_bucket_mb * (1 << 20)) // 4, int(bucket_cap_mb * (1 << 20)) // 4, int(last_bucket_mb * (1 << 20)) // 4)
        self._arrival, self._rebuilt = [], False
        self._plan(list(reversed(params)))
        for p in params:
            p.register_post_accumulate_grad_hook(self._on_grad)

    def _plan(self, ordered):
        """Cut ``ordered`` (parameters in the order their gradients arrive) into buckets.  The gradients that arrive LAST -- the stem
        and the first encoder stage -- get a small bucket of their own: the exchange of the final bucket is the part of the
        collective that no backward kernel can hide, and with 25 MB buckets it carried whatever arrived in the last third of
        backward (enqueued at 97 % of it: profiles/round4_j_ddp_bucket_timeline.md)."""
        self.buckets, cur, n = [], [], 0
        cap = self._caps[0]
        tail, tn = [], 0
        tail_cap = min(self._caps[2], self._caps[1] // 4)
        while len(ordered) > 1 and tn + ordered[-1].numel() <= tail_cap:
            tail.insert(0, ordered[-1])
            tn += ordered[-1].numel()
            ordered = ordered[:-1]
        for p in ordered:
            cur.append(p)
            n += p.numel()
            if n >= cap:
                self._close(cur, n)
                cur, n, cap = [], 0, self._caps[1]
        if cur:
            self._close(cur, n)
        if tail:
            self._close(tail, tn)
        self._where = {}
        for bi, b in enumerate(self.buckets):
            for p in b["params"]:
                self._where[p] = bi

    def _close(self, params, n):
        flat = torch.zeros(n, device=params[0].device, dtype=torch.float32)
        views, off = [], 0
        for p in params:
            views.append(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        self.buckets.append({"params": list(params), "flat": flat, "views": views, "ready": 0, "handle": None})

    def _on_grad(self, p):
        if not self._rebuilt:
            self._arrival.append(p)                   # first backward: remember the order the gradients arrive in
        b = self.buckets[self._where[p]]
        b["ready"] += 1
        if b["ready"] == len(b["params"]):
            torch._foreach_copy_(b["views"], [q.grad for q in b["params"]])
            if self.world > 1:
                b["flat"].mul_(1.0 / self.world)
            b["handle"] = self.dist.all_reduce(b["flat"], group=self.group, async_op=True)

    def finish(self):
        """After backward: wait for every bucket's exchange and hand the averaged gradients to the parameters."""
        for b in self.buckets:
            if b["ready"] != len(b["params"]):
                missing = len(b["params"]) - b["ready"]
                b["ready"] = 0
                raise RuntimeError(f"BucketedGradSync: {missing} parameter(s) of a bucket received no gradient in this backward "
                                   "(every trainable parameter must take part in every step)")
            b["handle"].wait()
            b["handle"], b["ready"] = None, 0
            for p, v in zip(b["params"], b["views"]):
                p.grad = v
        if not self._rebuilt:
            # every rank saw the same arrival order (same network, same autograd graph): the new plan is identical everywhere.  The
            # gradients of THIS step keep living in the old flat buffers (p.grad views above) until the optimizer has used them
            self._rebuilt = True
            if len(self._arrival) == len(self._where) and len(set(map(id, self._arrival))) == len(self._arrival):
                self._plan(self._arrival)
            self.arrival_order, self._arrival = self._arrival, []


GRAD_SYNC = os.environ.get("MLAGG_GRAD_SYNC", "bucketed")     # "ddp": torch's DistributedDataParallel on the device too


def wrap_ddp(model, device_index=None, bucket_cap_mb=25):
    """The data-parallel wrapper of the train step (reference nnUNetTrainer.py:205-207).  The never-used ``dummy_tensor``
    (reference T:1362) is frozen (``requires_grad`` False: only parameters that require a gradient are exchanged), so no
    unused-parameter search is needed (SURVEY finding 7a).
    Device parameters: the network itself comes back with a ``BucketedGradSync`` attached (``network._mlagg_grad_sync``; ``.module``
    is the network, as the reference's code expects of a DDP wrapper) -- ``train_step`` calls its ``finish()`` after backward.
    Host parameters (the gloo tier) and MLAGG_GRAD_SYNC=ddp: torch's DistributedDataParallel with gradient buckets as views."""
    dummy = getattr(model, "dummy_tensor", None)
    if isinstance(dummy, torch.nn.Parameter):
        dummy.requires_grad_(False)
    on_device = all(p.is_cuda for p in model.parameters())
    if on_device and GRAD_SYNC != "ddp":
        sync = BucketedGradSync(model, bucket_cap_mb=bucket_cap_mb)
        object.__setattr__(model, "_mlagg_grad_sync", sync)
        object.__setattr__(model, "module", model)          # not a registered sub-module: state_dict keys stay the network's own
        return model
    from torch.nn.parallel import DistributedDataParallel as DDP
    ids = None if device_index is None else [device_index]
    return DDP(model, device_ids=ids, bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True,
               broadcast_buffers=False)


def finish_grad_sync(network):
    """Wait for the bucketed gradient exchange of ``wrap_ddp`` (a no-op for plain and DistributedDataParallel networks)."""
    sync = getattr(network, "_mlagg_grad_sync", None)
    if sync is not None:
        sync.finish()


def set_deterministic(enabled=True):
    """Bit-reproducible train steps.  This package's kernels on the train path hold no float atomics (per-workgroup partials
    summed in a fixed order; round 3 removed the last ones: K9's loss statistics, K3 / K4's d(lambda) / d(subln) sums, the clip
    norm); what still differed between two runs on identical inputs were MIOpen solvers that accumulate with atomics (the 1x1 /
    transposed-convolution weight gradients and one data gradient: tools/find_nondeterminism.py, profiles/round3_nondeterminism_*).
    ``torch.backends.cudnn.deterministic`` is PyTorch's switch for MIOpen's deterministic-solvers-only attribute: with it all 524
    gradients of a 256 x 256 batch-10 step are bit-identical from run to run.  Not the default: it takes the tuned find-db's
    solver picks away from those layers."""
    torch.backends.cudnn.deterministic = bool(enabled)


def set_deep_supervision_enabled(network, enabled):
    """Reference T:94-99 writes the attribute on the DDP wrapper (SURVEY finding 7b); unwrap first."""
    getattr(network, "module", network).deep_supervision = enabled


# ------------------------------------------------------------------------------------------------
# step
# ------------------------------------------------------------------------------------------------
def train_step(network, optimizer, data, target: List[torch.Tensor], batch_dice=True, ddp=False, clip=12.0,
               loss_fn=None, grad_scaler=None):
    """One optimisation step on device-resident tensors; returns the detached loss tensor (the caller
    decides when to synchronise -- the reference's ``.cpu()`` per step, B:863, is a host sync).
    ``loss_fn(output, target)`` replaces the Dice + CE deep-supervision loss (the trainer plugin passes ``self.loss``).
    ``grad_scaler``: the reference's fp16 branch (B:853-858): scaled backward, unscale, clip, step, update -- for networks
    built with ``precision="fp16"``, whose 16-bit GEMM operands would flush small gradients to zero unscaled.  A
    ``torch.amp.GradScaler`` takes torch's path (``found_inf.item()`` on the host); a ``DeviceGradScaler`` the fused one (K35): scaled
    backward, then unscale, clip, skip-or-step and the new scale in the optimizer's own launches.  Under DDP every rank sees the
    same reduced gradients and so takes the same decision."""
    optimizer.zero_grad(set_to_none=True)
    output = network(data)
    loss = deep_supervision_loss(output, target, batch_dice, ddp) if loss_fn is None else loss_fn(output, target)
    if isinstance(grad_scaler, DeviceGradScaler):
        grad_scaler.scale(loss).backward()
        finish_grad_sync(network)
        grad_scaler.step(optimizer, max_norm=clip)
        grad_scaler.update()
        return loss.detach()
    if grad_scaler is not None:
        grad_scaler.scale(loss).backward()
        finish_grad_sync(network)
        grad_scaler.unscale_(optimizer)
        if isinstance(optimizer, ClipOptimizer):
            grad_scaler.step(optimizer, max_norm=clip)
        else:
            torch.nn.utils.clip_grad_norm_([p for p in network.parameters() if p.grad is not None], clip)
            grad_scaler.step(optimizer)
        grad_scaler.update()
        return loss.detach()
    loss.backward()
    finish_grad_sync(network)
    if isinstance(optimizer, ClipOptimizer):
        optimizer.step(max_norm=clip)                      # norm, clip coefficient and update on the device, two launches
    else:
        torch.nn.utils.clip_grad_norm_([p for p in network.parameters() if p.grad is not None], clip)
        optimizer.step()
    return loss.detach()


class GraphedTrainStep:
    """The whole train step (zero_grad, forward, loss, backward, clip, AdamW) captured once into a hipGraph
    and replayed: ~3400 kernel launches per step otherwise cost more host time than the MI355X needs to
    execute them.  Inputs are copied into static buffers; every HIP op of this package launches on the
    capturing stream and never allocates or synchronises, so it records cleanly.  Single-process use: the DDP path stays eager.
    Measured in round 3 with one RCCL rank (bench.py MLAGG_FORCE_DDP=1): the eager DDP step runs (44.7 vs 43.5 ms per step); capturing
    it -- PyTorch's documented DDP-in-graph recipe, 11 side-stream warm-ups -- ends in a segmentation fault inside the capture on this
    PyTorch 2.10 / ROCm 7.0 build (AccumulateGrad nodes stashed by DDP on another stream, then a crash in the RCCL work enqueue:
    profiles/round3_ddp_graph_capture_segfault.log), so a DistributedDataParallel network is refused here.
    One captured step per optimizer: the graph reads ClipAdamW's pointer table for captured steps, and a second capture whose
    gradients sit at other addresses would redirect the first graph's update, so ClipAdamW refuses it.  Eager ``train_step``
    calls with the same optimizer may be mixed with replays freely.
    ``grad_scaler``: a ``DeviceGradScaler`` -- the fp16 step with loss scaling (K35) is captured whole; its scale, growth tracker and
    the optimizer's step counter advance inside the replays."""

    def __init__(self, network, optimizer, data, target, batch_dice=True, clip=12.0, warmup=3, loss_fn=None, grad_scaler=None):
        if grad_scaler is not None and not isinstance(grad_scaler, DeviceGradScaler):
            raise RuntimeError("GraphedTrainStep: only a DeviceGradScaler can be captured (torch.amp.GradScaler.step reads found_inf "
                               "on the host)")
        if isinstance(network, torch.nn.parallel.DistributedDataParallel) or getattr(network, "_mlagg_grad_sync", None) is not None:
            raise RuntimeError("GraphedTrainStep: a DistributedDataParallel network cannot be captured on this build "
                               "(segmentation fault inside the capture); run the data-parallel step eagerly")
        self.data = data.clone()
        self.target = [t.clone() for t in target]
        body = lambda: train_step(network, optimizer, self.data, self.target, batch_dice, False, clip, loss_fn=loss_fn,  # noqa: E731
                                  grad_scaler=grad_scaler)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()                      # nothing of the warm-up is in flight when the capture rewrites host tables
        optimizer.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = body()
        self.optimizer = optimizer

    def __call__(self, data=None, target=None):
        if data is not None:
            self.data.copy_(data, non_blocking=True)
        if target is not None:
            for dst, src in zip(self.target, target):
                dst.copy_(src, non_blocking=True)
        if isinstance(self.optimizer, ClipOptimizer):
            self.optimizer.sync_lr()                  # the learning rate the host holds NOW governs this replay
        self.graph.replay()
        # the replay rewrote the parameters through raw pointers and ran no host code: stacked weights and weight images that an
        # eager forward built earlier are one step behind, and no version counter says so
        from . import ops
        ops.invalidate_weight_images()
        return self.loss


def synthetic_batch(batch, in_ch, H, W, n_cls, seed=1234, device="cpu"):
    """Benchmark inputs of the reference's nnUNetTrainerBenchmark_5epochs_noDataLoading.py:16-22."""
    g = torch.Generator().manual_seed(seed)
    data = torch.rand(batch, in_ch, H, W, generator=g)
    target = [torch.round(torch.rand(batch, 1, H >> s, W >> s, generator=g) * (n_cls - 1)) for s in range(5)]
    return data.to(device), [t.to(device) for t in target]
