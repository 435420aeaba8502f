"""CPU: the C-ABI library loads and exports every symbol include/mlagg_hip.h declares (no compute
calls: there is no GPU here), argument validation, and the host logic around the hot path."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    text = open(os.path.join(ROOT, "include", "mlagg_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared_symbols():
    return sorted(set(re.findall(r"\b(mlagg_[a-z0-9_]+)\s*\(", _header_text())))


def _declarations():
    """name -> (return type, parameter count) of every declaration, read here independently of _lib's parser: the return type is
    what precedes the name on its line, the parameters are counted by their commas."""
    text = _header_text()
    out = {}
    for m in re.finditer(r"\b(mlagg_[a-z0-9_]+)\s*\(([^)]*)\)", text):
        ret = text[text.rfind("\n", 0, m.start()) + 1:m.start()]
        params = m.group(2).strip()
        out[m.group(1)] = (" ".join(ret.replace("*", " *").split()), 0 if params in ("", "void") else params.count(",") + 1)
    return out


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as G
    G.build()
    from mlagg_unet_amd import _lib
    handle = ctypes.CDLL(_lib.SO_PATH)
    declared = _declared_symbols()
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in mlagg_hip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert set(_lib.SIGNATURES) == set(declared)
    restypes = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
    for name, (ret, nparams) in _declarations().items():
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nparams, f"{name}: {len(args)} ctypes arguments for {nparams} declared parameters"
        assert res is restypes[ret], f"{name}: restype {res} for the declared return type {ret!r}"
    lib = _lib.lib()
    assert lib.mlagg_version().startswith(b"mlagg_hip")
    assert b"unsupported" in lib.mlagg_error_string(-1)
    # size queries are pure host arithmetic
    assert lib.mlagg_selscan_state_floats(10, 384, 21760, 16) == 10 * 340 * 384 * (16 + 1 + 7 * 16)   # chunk states, sums, 8-step tile states
    assert lib.mlagg_local_attn_bwd_workspace_floats(2, 8, 8, 1) >= 2 * 64 * 76
    names = [lib.mlagg_profile_kernel_name(i).decode() for i in range(lib.mlagg_profile_kernel_count())]
    assert "selscan_bwd_group_kernel" in names and "tok_bwd_group_kernel" in names and len(set(names)) == len(names)


def test_ops_refuse_cpu_tensors_and_unsupported_arguments():
    """No CPU / eager fallback: the product ops raise instead of computing elsewhere."""
    from mlagg_unet_amd import ops
    u = torch.zeros(1, 8, 16)
    with pytest.raises(RuntimeError):
        ops.selective_scan_fn(u, u, torch.zeros(8, 16), torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))
    with pytest.raises(RuntimeError):
        ops.selective_scan_fn(u, u, torch.zeros(8, 16), torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16),
                              z=torch.zeros(1, 8, 16))
    with pytest.raises(RuntimeError):
        ops.dwconv3x3_nlc(torch.zeros(1, 4, 8), torch.zeros(8, 1, 3, 3), None, 2, 2)
    with pytest.raises(RuntimeError):
        ops.local_diff_attn(torch.zeros(1, 4, 48), torch.zeros(1, 4, 96), torch.zeros(()), torch.ones(48),
                            torch.zeros(48, 1, 3, 3), torch.zeros(48), 2, 2, 1, 24 ** -0.5)


def test_product_model_has_reference_state_dict_keys():
    from mlagg_unet_amd import model
    from oracle import mlagg_oracle as O
    m = model.build_network_architecture((64, 64), 1, 14)
    o = O.build_reference_config_model((64, 64))
    assert list(sorted(m.state_dict())) == list(sorted(o.state_dict()))
    assert sum(p.numel() for p in m.parameters()) == 27_095_447
    for k, v in o.state_dict().items():
        assert m.state_dict()[k].shape == v.shape, k
    m2 = model.build_network_architecture((64, 64), 1, 14, enable_deep_supervision=False)
    assert not any(k.startswith("out_1") for k in m2.state_dict())


def test_split_batch_size_never_zero_or_negative():
    from mlagg_unet_amd import trainer
    assert trainer.split_batch_size(10, 8) == [2, 2, 1, 1, 1, 1, 1, 1]      # reference gives (2,2,2,2,2,0,-2,-4)
    assert trainer.split_batch_size(80, 8) == [10] * 8
    assert sum(trainer.split_batch_size(13, 4)) == 13
    with pytest.raises(RuntimeError):
        trainer.split_batch_size(3, 4)


def test_cosine_schedule_matches_timm_formula():
    from mlagg_unet_amd import trainer
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], 5e-4)
    s = trainer.CosineLRSchedule(opt, t_initial=500, lr_min=1e-6, warmup_t=10, warmup_lr_init=1e-4)
    s.step(0)
    assert abs(opt.param_groups[0]["lr"] - 1e-4) < 1e-12
    s.step(5)
    assert abs(opt.param_groups[0]["lr"] - (1e-4 + 5 * (5e-4 - 1e-4) / 10)) < 1e-12
    s.step(250)
    assert abs(opt.param_groups[0]["lr"] - (1e-6 + 0.5 * (5e-4 - 1e-6))) < 1e-9
    s.step(500)
    assert abs(opt.param_groups[0]["lr"] - 1e-6) < 1e-12


@pytest.mark.parametrize("capturable", [False, True])
def test_clip_adamw_learning_rate_is_a_host_float_a_training_loop_can_log(capturable):
    """What the epoch-start hook of a host training loop does with ``param_groups[0]["lr"]`` after the schedule's step: round it
    with numpy for the log line, keep it in a logger that is pickled with the checkpoint.  A device tensor there fails both; the
    capturable form keeps its device copy outside ``param_groups``, so optimizer checkpoints hold no tensor hyper-parameter."""
    import pickle
    import numpy as np
    from mlagg_unet_amd import trainer
    p = torch.nn.Parameter(torch.zeros(3))
    opt = trainer.ClipAdamW([p], 5e-4, eps=1e-4, weight_decay=3e-5, capturable=capturable)
    sched = trainer.CosineLRSchedule(opt, t_initial=500, lr_min=1e-6, warmup_t=10, warmup_lr_init=1e-4)
    log = []
    for epoch in (0, 5, 250):
        sched.step(epoch)
        lr = opt.param_groups[0]["lr"]
        assert type(lr) is float and float(lr) == sched.lr_at(epoch, 5e-4)
        shown = np.round(lr, decimals=5)
        assert isinstance(shown, float) and np.isfinite(shown) and abs(shown - lr) <= 5e-6
        log.append(shown)
        assert pickle.loads(pickle.dumps(log)) == log
        groups = opt.state_dict()["param_groups"]
        assert not any(torch.is_tensor(v) for g in groups for v in g.values())
    opt.load_state_dict(opt.state_dict())
    assert type(opt.param_groups[0]["lr"]) is float and opt.param_groups[0]["lr"] == sched.lr_at(250, 5e-4)


def test_capturable_clip_adamw_loads_moments_into_the_tensors_it_has():
    """A captured graph holds the addresses of the moment tensors: ``load_state_dict`` of the capturable form copies the loaded
    values into the existing tensors (the launch-argument form takes the loaded tensors, as torch's optimizers do)."""
    import copy
    from mlagg_unet_amd import trainer
    for capturable in (True, False):
        ps = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2, 3))]
        opt = trainer.ClipAdamW(ps, 5e-4, capturable=capturable)
        for i, p in enumerate(ps):
            st = opt._state_of(p)
            st["exp_avg"].fill_(1.0 + i)
            st["exp_avg_sq"].fill_(10.0 + i)
        sd = copy.deepcopy(opt.state_dict())
        for i in range(2):
            sd["state"][i]["step"] = torch.tensor(7.0)
            sd["state"][i]["exp_avg"] += 0.5
        sd["param_groups"][0]["lr"] = 3e-4
        ptrs = [opt.state[p][k].data_ptr() for p in ps for k in ("exp_avg", "exp_avg_sq")]
        opt.load_state_dict(sd)
        assert ([opt.state[p][k].data_ptr() for p in ps for k in ("exp_avg", "exp_avg_sq")] == ptrs) == capturable
        for i, p in enumerate(ps):
            assert torch.equal(opt.state[p]["exp_avg"], torch.full_like(p, 1.5 + i))
            assert torch.equal(opt.state[p]["exp_avg_sq"], torch.full_like(p, 10.0 + i))
        assert opt.steps_done() == 7 and opt.param_groups[0]["lr"] == 3e-4
        assert float(opt.state_dict()["state"][1]["step"]) == 7.0


def test_product_loss_equals_oracle_loss_on_cpu():
    from mlagg_unet_amd import trainer
    from oracle import mlagg_oracle as O
    g = torch.Generator().manual_seed(3)
    outs = [torch.randn(2, 6, 32 >> s, 32 >> s, generator=g, requires_grad=True) for s in range(5)]
    tg = [torch.round(torch.rand(2, 1, 32 >> s, 32 >> s, generator=g) * 5) for s in range(5)]
    for bd in (True, False):
        a = trainer.deep_supervision_loss(outs, tg, batch_dice=bd)
        b = O.deep_supervision_loss(outs, tg, batch_dice=bd)
        assert abs(float(a.detach()) - float(b.detach())) < 1e-6
        ga = torch.autograd.grad(a, outs)
        gb = torch.autograd.grad(b, outs)
        for x, y in zip(ga, gb):
            assert torch.allclose(x, y, atol=1e-7)


def test_product_and_tools_never_import_the_oracle():
    """oracle/ is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import it
    (the product path must not route through a CPU restatement)."""
    import ast
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    offenders = []
    for path in glob.glob(os.path.join(root, "mlagg-unet_amd", "**", "*.py"), recursive=True) + \
            glob.glob(os.path.join(root, "tools", "**", "*.py"), recursive=True) + [os.path.join(root, "mlagg_unet_amd.py")]:
        tree = ast.parse(open(path).read())
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            if any(n == "oracle" or n.startswith("oracle.") for n in names):
                offenders.append(os.path.relpath(path, root))
    assert not offenders, offenders
    # bench.py and __graft_entry__.py: the import sits inside cpu_baseline's helper / smoke() only
    for name, allowed in (("bench.py", {"_oracle_step_seconds", "cpu_baseline_3d"}), ("__graft_entry__.py", {"smoke"})):
        tree = ast.parse(open(os.path.join(root, name)).read())
        for fn in [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)]:
            uses = any(isinstance(n, ast.ImportFrom) and (n.module or "").startswith("oracle") for n in ast.walk(fn))
            assert not uses or fn.name in allowed, (name, fn.name)
        top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
        assert not any(isinstance(n, ast.ImportFrom) and (n.module or "").startswith("oracle") for n in top), name


def test_committed_tuning_tables_are_well_formed():
    """The MIOpen find-db and the TunableOp GEMM table that bench.py loads: present, parseable, made for gfx950."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gemm = glob.glob(os.path.join(root, "mlagg-unet_amd", "gemm_db", "*.csv"))
    assert len(gemm) == 1
    lines = open(gemm[0]).read().strip().split("\n")
    assert any(ln.startswith("Validator,GCN_ARCH_NAME,gfx950") for ln in lines)
    rows = [ln.split(",") for ln in lines if not ln.startswith("Validator")]
    assert len(rows) >= 30 and all(len(r) == 4 and float(r[3]) > 0 for r in rows)
    ufdb = glob.glob(os.path.join(root, "mlagg-unet_amd", "miopen_db", "*.ufdb.txt"))
    assert len(ufdb) == 1 and "gfx950" in os.path.basename(ufdb[0])
    assert all("=" in ln for ln in open(ufdb[0]).read().strip().split("\n"))
    from mlagg_unet_amd import gemm_tuning
    assert gemm_tuning.use_tuned_gemms(enabled=False) is None
