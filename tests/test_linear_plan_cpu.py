"""CPU: the kernel each product of every token-major projection runs on (ops.linear_plan), and where ops.mlp fuses a block's Mlp
(MlpFn), in each compute dtype -- every distinct (tokens, out, in) of the 2-D network at 256 x 256 and 224 x 224 (batch 10) and
512 x 640 (batch 4), MLPs, stacked projections and the padded x_proj included, and of the 3-D network at 96 x 160 x 160 (batch 2).
An entry is "forward/data gradient/weight gradient" ("lib": that product on the library)."""
import types

import pytest
import torch

from mlagg_unet_amd import ops

CDTS = (torch.float32, torch.bfloat16, torch.float16)
PRECISION = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}

# (tokens M, out O, in I, fp32, bf16, fp16, fp32 with the tuned GEMM table loaded)
LINEAR = [
    (435200,   48,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (435200,   96,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (435200,  144,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (327680,   48,  128, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (327680,   96,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (327680,   96,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (327680,  144,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (327680,  192,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (327680,  256,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (217600,   48,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (217600,   96,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (217600,  144,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (166600,   48,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (166600,   96,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (166600,  144,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (163840,   48,  128, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (163840,   96,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (163840,   96,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (163840,  144,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (163840,  192,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (163840,  256,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (125440,   48,  128, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (125440,   96,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (125440,   96,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (125440,  144,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (125440,  192,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (125440,  256,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 81920,   48,  128, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 81920,  192,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 81920,  192,  384, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 81920,  256,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 81920,  288,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 81920,  384,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 40960,   48,  128, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 40960,  192,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 40960,  192,  384, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 40960,  256,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 40960,  288,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 40960,  384,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 31360,   48,  128, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 31360,  192,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 31360,  192,  384, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 31360,  256,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 31360,  288,   96, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 31360,  384,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 20480,   48,  128, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 20480,  256,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 20480,  384,  384, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 20480,  384,  768, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 20480,  576,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 20480,  768,  384, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 10240,   48,  128, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 10240,  256,   48, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 10240,  384,  384, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 10240,  384,  768, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 10240,  576,  192, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    ( 10240,  768,  384, 'K5x3/K5x3/K5w'     , 'K5/K5/K5w'         , 'K5/K5/K5w'         , 'K5x3/K5x3/K5w'     ),
    (  7840,   48,  128, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  7840,  256,   48, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  7840,  384,  384, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  7840,  384,  768, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  7840,  576,  192, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  7840,  768,  384, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  5120,   48,  128, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  5120,  256,   48, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  5120,  768,  768, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  5120,  768, 1536, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  5120, 1152,  384, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  5120, 1536,  768, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  2560,   48,  128, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  2560,  256,   48, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  2560,  768,  768, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  2560,  768, 1536, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  2560, 1152,  384, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  2560, 1536,  768, 'K5x3/K5x3/K5w'     , 'lib/lib/K5w'       , 'lib/lib/K5w'       , 'K5x3/K5x3/lib'     ),
    (  1960,   48,  128, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1960,  256,   48, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1960,  768,  768, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1960,  768, 1536, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1960, 1152,  384, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1960, 1536,  768, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1280,   96,   48, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1280,  192,   96, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1280,  384,  192, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (  1280,  768,  384, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (   640,   96,   48, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (   640,  192,   96, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (   640,  384,  192, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (   640,  768,  384, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (   490,   96,   48, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (   490,  192,   96, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (   490,  384,  192, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
    (   490,  768,  384, 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       , 'lib/lib/lib'       ),
]

# the 3-D network's projections (fp32)
LINEAR_3D = [
    (4915200,   32,   64, 'K5x3/K5x3/K5w'),
    (4915200,   48,   64, 'K5x3/K5x3/K5w'),
    (4915200,   64,   32, 'K5x3/K5x3/K5w'),
    ( 614400,   64,  128, 'K5x3/K5x3/K5w'),
    ( 614400,   72,  128, 'K5x3/K5x3/K5w'),
    ( 614400,  128,   64, 'K5x3/K5x3/K5w'),
    (  76800,  120,  256, 'K5x3/K5x3/K5w'),
    (  76800,  128,  256, 'K5x3/K5x3/K5w'),
    (  76800,  128,  512, 'K5x3/K5x3/K5w'),
    (  76800,  256,  128, 'K5x3/K5x3/K5w'),
    (  76800,  512,  128, 'K5x3/K5x3/K5w'),
    (   9600,  216,  512, 'K5x3/K5x3/K5w'),
    (   9600,  256,  512, 'K5x3/K5x3/K5w'),
    (   9600,  256, 1024, 'K5x3/K5x3/K5w'),
    (   9600,  512,  256, 'K5x3/K5x3/K5w'),
    (   9600, 1024,  256, 'K5x3/K5x3/K5w'),
    (   1200,  264,  640, 'lib/lib/lib'),
    (   1200,  320,  640, 'lib/lib/lib'),
    (   1200,  320, 1280, 'lib/lib/lib'),
    (   1200,  640,  320, 'lib/lib/lib'),
    (   1200, 1280,  320, 'lib/lib/lib'),
    (    300,  264,  640, 'lib/lib/lib'),
    (    300,  320,  640, 'lib/lib/lib'),
    (    300,  320, 1280, 'lib/lib/lib'),
    (    300,  640,  320, 'lib/lib/lib'),
    (    300, 1280,  320, 'lib/lib/lib'),
]

# ops.mlp of an Mlp block: (tokens M, in I, hidden H, out O, MlpFn in fp32, bf16, fp16)
MLP = [
    (327680,   96,  192,   96, True , False, False),
    (163840,   96,  192,   96, True , False, False),
    (125440,   96,  192,   96, True , False, False),
    ( 81920,  192,  384,  192, True , False, False),
    ( 40960,  192,  384,  192, True , False, False),
    ( 31360,  192,  384,  192, True , False, False),
    ( 20480,  384,  768,  384, True , False, False),
    ( 10240,  384,  768,  384, True , False, False),
    (  7840,  384,  768,  384, True , False, False),
    (  5120,  768, 1536,  768, True , False, False),
    (  2560,  768, 1536,  768, True , False, False),
    (  1960,  768, 1536,  768, False, False, False),
]


def _fmt(plan):
    return "/".join(v or "lib" for v in plan)


@pytest.mark.parametrize("row", LINEAR, ids=lambda r: "{}x{}x{}".format(*r[:3]))
def test_linear_plan_table(row, monkeypatch):
    M, O, I = row[:3]
    for cdt, want in zip(CDTS, row[3:6]):
        assert _fmt(ops.linear_plan(M, O, I, cdt, True)) == want, (cdt, want)
    monkeypatch.setattr(ops, "GEMM_TABLE_LOADED", [True])
    assert _fmt(ops.linear_plan(M, O, I, torch.float32, True)) == row[6]


@pytest.mark.parametrize("row", LINEAR_3D, ids=lambda r: "{}x{}x{}".format(*r[:3]))
def test_linear_plan_table_3d(row):
    assert _fmt(ops.linear_plan(*row[:3], torch.float32, True)) == row[3]


def test_linear_plan_reads_thresholds_at_each_call(monkeypatch):
    assert ops.linear_plan(1960, 768, 768, torch.float32, True) == (None, None, None)
    monkeypatch.setattr(ops, "X3_MIN_ROWS", 512)
    assert ops.linear_plan(1960, 768, 768, torch.float32, True) == ("K5x3", "K5x3", None)
    monkeypatch.setattr(ops, "WGRAD_MIN_ROWS", 1024)
    assert ops.linear_plan(1960, 768, 768, torch.float32, True) == ("K5x3", "K5x3", "K5w")


def test_linear_plan_of_host_tensors_is_the_library():
    for cdt in CDTS:
        assert ops.linear_plan(327680, 96, 96, cdt, False) == (None, None, None)


@pytest.mark.parametrize("row", MLP, ids=lambda r: "{}x{}x{}x{}".format(*r[:4]))
def test_mlp_fusion_table(row, monkeypatch):
    M, I, H, O = row[:4]
    monkeypatch.setattr(ops, "MlpFn", types.SimpleNamespace(apply=lambda *a: "MlpFn"))
    monkeypatch.setattr(ops, "linear", lambda x, w, b=None, plan=None: torch.zeros(1))
    x = types.SimpleNamespace(is_cuda=True, numel=lambda: M * I)
    for cdt, want in zip(CDTS, row[4:]):
        with ops.compute_precision(PRECISION[cdt]):
            got = ops.mlp(x, torch.empty(H, I), None, torch.empty(O, H), None)
        assert (isinstance(got, str) and got == "MlpFn") == want, (cdt, want)
