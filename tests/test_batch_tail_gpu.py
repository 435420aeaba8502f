"""GPU: K36 (ops.batch_tail on device tensors) against the host composition (the same function on CPU tensors, tests/test_batch_tail_cpu.py
ties that to the reference's transforms).  Copies, zeros and 0 / 1 only: every comparison is torch.equal."""
import pytest
import torch

import _batch_tail_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("seg_dtype", [torch.float32, torch.int16], ids=["fp32", "int16"])
@pytest.mark.parametrize("mode", list(C.MODES))
@pytest.mark.parametrize("name", list(C.GEOMETRIES))
def test_kernel_equals_host_composition(name, mode, seg_dtype):
    """Per geometry, target mode and seg type: mask_channels empty / a strict subset / all, one and two seg channels.  Unlisted data
    channels keep their bits, a repeat call gives identical bits, and K36 reads only channel 0 of seg."""
    from mlagg_unet_amd import ops
    regions, ignore = C.MODES[mode]
    sizes = C.level_sizes(name)
    n_channels = C.GEOMETRIES[name][1]
    for seg_channels in (1, 2):
        data, seg = C.batch(name, seg_dtype, seg_channels)
        for mask in C.mask_choices(n_channels):
            want_data, want = ops.batch_tail(data.clone(), seg, sizes, mask, regions, ignore)
            dev_data = data.to(DEV)
            got_data, got = ops.batch_tail(dev_data, seg.to(DEV), sizes, mask, regions, ignore)
            assert got_data is dev_data and torch.equal(got_data.cpu(), want_data), (seg_channels, mask)
            assert [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
            for lvl, (g, w) in enumerate(zip(got, want)):
                assert g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and torch.equal(g.cpu(), w), (seg_channels, mask, lvl)
            for c in range(n_channels):
                if c not in mask:
                    assert torch.equal(got_data[:, c].cpu(), data[:, c])
            if mask:
                assert not torch.equal(want_data, data)                      # the case does mask something
            _, again = ops.batch_tail(data.to(DEV), seg.to(DEV), sizes, mask, regions, ignore)
            assert all(torch.equal(a, g) for a, g in zip(again, got))
    if regions is not None:
        assert got[0].shape[1] == len(regions) + (ignore is not None) and set(got[0].unique().tolist()) == {0.0, 1.0}
    else:
        assert float(got[0].min()) == 0.0 and float(got[0].max()) == 300.0   # -1 is gone, a label above the region table is copied


@pytest.mark.parametrize("name", ["2d_odd_rows", "3d_scales"])
def test_label_mode_is_targets_from_seg_on_the_device(name):
    from mlagg_unet_amd import dataloading, ops
    _, _, _, levels = C.GEOMETRIES[name]
    data, seg = C.batch(name, torch.float32, 1)
    seg = seg.to(DEV)
    want = dataloading.targets_from_seg(seg, levels) if isinstance(levels, int) else dataloading.targets_from_seg(seg, ds_scales=levels)
    _, got = ops.batch_tail(data.to(DEV), seg, C.level_sizes(name))
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_given_tables_gather_and_misaligned_bases():
    """Explicit index tables (a reversal and a repeat), and a batch whose tensors start 4 bytes into their allocation: the vector
    paths need 16-byte bases, so the label loads and the mask's stores of that call are scalar ones."""
    from mlagg_unet_amd import ops
    data, seg = C.batch("2d_five_halvings", torch.float32, 1)
    rows = torch.arange(23, -1, -1, dtype=torch.int32)
    cols = torch.tensor([0, 0, 39, 5, 6, 7, 8], dtype=torch.int32)
    tables = [[None, None], [rows, cols], [None, cols]]
    sizes = [(24, 40), (24, 7), (24, 7)]
    _, want = ops.batch_tail(data.clone(), seg, sizes, (), C.REGIONS_3, None, tables=tables)
    assert torch.equal(want[1][0, 2, 0, 2], (seg[0, 0, 23, 39] == 3).float())
    dev_tables = [[None if t is None else t.to(DEV) for t in level] for level in tables]
    _, got = ops.batch_tail(data.to(DEV), seg.to(DEV), sizes, (), C.REGIONS_3, None, tables=dev_tables)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))

    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        flat[1:] = t.reshape(-1).to(DEV)
        return flat[1:].view(t.shape)

    sizes = C.level_sizes("2d_five_halvings")
    want_data, want = ops.batch_tail(data.clone(), seg, sizes, (0, 1), C.REGIONS_8, C.IGNORE_8)
    got_data, got = ops.batch_tail(shifted(data), shifted(seg), sizes, (0, 1), C.REGIONS_8, C.IGNORE_8)
    assert got_data.data_ptr() % 16 == 4 and torch.equal(got_data.cpu(), want_data)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


def test_bad_arguments_raise():
    from mlagg_unet_amd import dataloading, ops
    data, seg = (t.to(DEV) for t in C.batch("2d_odd_rows", torch.float32, 1))
    sizes = C.level_sizes("2d_odd_rows")
    short = [[None, None], [dataloading.nearest_index(23, 11).to(DEV), dataloading.nearest_index(37, 18)[:-1].to(DEV)], [None, None]]
    with pytest.raises(RuntimeError):
        ops.batch_tail(data, seg, sizes, tables=short)                       # a table shorter than its level
    host_tables = [[None, None], [dataloading.nearest_index(23, 11), dataloading.nearest_index(37, 18)], [None, None]]
    with pytest.raises(RuntimeError):
        ops.batch_tail(data, seg, sizes[:2], tables=host_tables[:2])         # tables that are not on the device
    for kwargs in (dict(mask_channels=[3]), dict(mask_channels=[-1]), dict(regions=[(i,) for i in range(33)]), dict(ignore_label=-3)):
        with pytest.raises(RuntimeError):
            ops.batch_tail(data, seg, sizes, **kwargs)
    for bad_sizes in ([], [sizes[0]] * 9):                                   # L = 0, L > 8
        with pytest.raises(RuntimeError):
            ops.batch_tail(data, seg, bad_sizes)
    with pytest.raises(RuntimeError):
        ops.batch_tail(data.transpose(2, 3), seg.transpose(2, 3), [(37, 23)])    # non-contiguous
    with pytest.raises(RuntimeError):
        ops.batch_tail(data, seg.cpu(), sizes)
    before = data.clone()
    ops.batch_tail(data, seg, sizes)                                         # and a good call after the refused ones
    assert torch.equal(data, before)
