"""TEST INFRASTRUCTURE: the seeded inputs of tests/golden/loss_variants.npz, shared by its generator
(tests/golden/make_golden_loss_variants.py) and by tests/test_loss_variants_cpu.py.  Only the seeds are stored in the fixture."""
import torch

LEVEL_SHAPES = ((24, 20), (12, 10), (6, 5))           # three deep-supervision levels, batch 2
BATCH = 2
SEED = 97
IGNORE = 5                                            # the ignore case: 6-channel logits, label 5 is the ignore label
# variant -> does it hold a Dice term (stored for batch_dice True and False)
VARIANTS = {"topk10": False, "topk10_ls01": False, "dice_topk10": True, "dice": True, "ce": False, "dice_ce_nosmooth": True}


def inputs(ignore):
    """-> (logits per level (2, C, H, W) = 2 randn, label maps per level (2, 1, H, W) float), C = 6 with labels 0 .. 5 in the ignore
    case (about a sixth of the pixels carry the ignore label 5), else C = 5 with labels 0 .. 4."""
    g = torch.Generator().manual_seed(SEED + (1 if ignore else 0))
    C = 6 if ignore else 5
    logits = [2 * torch.randn(BATCH, C, h, w, generator=g) for h, w in LEVEL_SHAPES]
    labels = [torch.randint(0, C, (BATCH, 1, h, w), generator=g).float() for h, w in LEVEL_SHAPES]
    return logits, labels


def cases():
    """(variant, batch_dice, ignore) of every stored result"""
    return [(v, bd, ign) for ign in (False, True) for v, dice in VARIANTS.items() for bd in ((True, False) if dice else (True,))]


def tag(variant, batch_dice, ignore):
    return f"{variant}/bd{int(batch_dice)}/{'ignore' if ignore else 'plain'}"
