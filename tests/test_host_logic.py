"""CPU: host-side mirror of the reference interface (no GPU needed): module layout, error behaviour,
PSF taps, synthetic dataset contract, shard arithmetic."""
import copy
import io
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from oracle import sif_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sifsr():
    import sifsr as pkg
    return pkg


def test_model_container_matches_reference_state_dict(sifsr, golden):
    m = sifsr.ModelB_2(in_channels=2, downchannels=[16, 32, 64, 128], padding_mode="replicate", activation="ReLU",
                       bilinear=1, n_bridge_blocks=1)
    spec = [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()]
    assert spec == golden["state_dict_spec"]
    assert [n for n, _ in m.named_parameters()] == O.param_names()
    assert (m.in_channels, m.downchannels, m.padding, m.activation, m.upfactor, m.bridge) == \
           (2, [16, 32, 64, 128], "replicate", "ReLU", 2, 1)
    m.load_state_dict(O.synthetic_state(1), strict=True)
    assert isinstance(m.db1.downsampling, torch.nn.AvgPool2d) and isinstance(m.ub1.up, torch.nn.Upsample)


def test_unsupported_options_raise(sifsr):
    for bad in (dict(padding_mode="zeros"), dict(activation="Serf"), dict(bilinear=False), dict(downchannels=[8, 16, 32, 64])):
        with pytest.raises(NotImplementedError):
            sifsr.ModelB_2(2, **bad)
    with pytest.raises(NotImplementedError):
        sifsr.ModelB_2(3)


def test_no_cpu_fallback(sifsr):
    m = sifsr.ModelB_2(2)
    with pytest.raises(sifsr.SifsrError):
        m(torch.zeros(1, 2, 256, 256))
    x = torch.zeros(1, 1, 256, 256)
    for fn in (sifsr.downscale_LST_SR_to_LR, sifsr.get_output_ftm, sifsr.sobel_bank):
        with pytest.raises(sifsr.SifsrError):
            fn(x)
    with pytest.raises(sifsr.SifsrError):
        sifsr.sif_loss("sr2", x, torch.zeros(1, 1, 64, 64), x, 0.0, 1.0, 0.5, -0.25)
    with pytest.raises(NotImplementedError):
        sifsr.downscale_LST_SR_to_LR(x, deci_type="norm-L4")
    with pytest.raises(NotImplementedError):
        sifsr.get_output_ftm(x, factor=2)


def test_product_never_imports_oracle(sifsr):
    import os
    root = os.path.dirname(sifsr.__file__)
    for dp, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "sif_oracle" not in txt and "import oracle" not in txt and "from oracle" not in txt, f


def test_pickle_and_deepcopy_on_cpu(sifsr):
    m = sifsr.ModelB_2(2)
    m.load_state_dict(O.synthetic_state(2))
    m2 = pickle.loads(pickle.dumps(m))
    m3 = copy.deepcopy(m)
    for a, b, c in zip(m.state_dict().values(), m2.state_dict().values(), m3.state_dict().values()):
        assert torch.equal(a, b) and torch.equal(a, c)
    buf = io.BytesIO(); torch.save(m.state_dict(), buf); buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    assert list(sd.keys()) == [n for n, _, _ in O.state_dict_spec()]


def test_psf_taps(sifsr, golden):
    for mtf in (0.1, 0.25):
        t = sifsr.sif_ops.psf_taps_1d(mtf)
        np.testing.assert_allclose(t, golden["cases"][f"psf_{mtf}"]["taps1d"], rtol=0, atol=1e-15)
        k = np.array(golden["cases"][f"psf_{mtf}"]["kernel9x9"], dtype=np.float64).reshape(9, 9)   # the reference's kernel
        assert np.abs(np.outer(t, t) - k).max() < 2e-8
    with pytest.raises(NotImplementedError):
        sifsr.sif_ops._taps_c(0.1, 4, 3)


def test_synthetic_dataset_contract(sifsr):
    ds = sifsr.ModisDatasetB(None, transf="norm", split="Train", time="Both", length=5)
    assert len(ds) == 5 and set(ds.stats) == {"mean_lst", "std_lst", "mean_ndvi", "std_ndvi"}
    lst, lst_up, ndvi = ds[3]
    assert lst.shape == (1, 64, 64) and lst_up.shape == (1, 256, 256) and ndvi.shape == (1, 256, 256)
    assert lst.dtype == lst_up.dtype == ndvi.dtype == np.float32
    assert np.array_equal(ds[3][0], lst) and not np.array_equal(ds[2][0], lst)
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=2)))
    assert [tuple(t.shape) for t in batch] == [(2, 1, 64, 64), (2, 1, 256, 256), (2, 1, 256, 256)]
    with pytest.raises(IndexError):
        ds[5]


def test_shard_range_covers_everything(sifsr):
    from sifsr.distributed import shard_range
    for n in (0, 1, 7, 64, 324):
        for w in (1, 2, 3, 8):
            r = [shard_range(n, k, w) for k in range(w)]
            assert r[0][0] == 0 and r[-1][1] == n
            assert all(r[i][1] == r[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in r]
            assert max(sizes) - min(sizes) <= 1


def test_tile_granule(sifsr):
    lst = torch.arange(130 * 200, dtype=torch.float32).view(130, 200)
    ndvi = torch.zeros(520, 800)
    t, n, pos = sifsr.predict.tile_granule(lst, ndvi)
    assert t.shape == (6, 1, 64, 64) and n.shape == (6, 1, 256, 256)        # ragged edges skipped (predict.py:95)
    assert pos == [(0, 0), (0, 64), (0, 128), (64, 0), (64, 64), (64, 128)]
    assert torch.equal(t[4, 0], lst[64:128, 64:128])


def test_dropin_modules_cover_the_reference_scripts_names():
    """dropin/{model,dataset,utils}.py must offer every name the reference's three training scripts and predict.py take
    from ``model`` / ``dataset`` / ``utils`` (SURVEY.md §8 b).  The list below is what an ``ast`` reading of those four
    scripts gives (``from model/dataset import ...`` and every ``us.<name>`` attribute), less the GDAL HDF readers of
    predict.py (``read_LST``, ``read_NIRRED``, ``compute_NDVI``: out of scope); it is committed, so the check needs
    nothing outside the repository."""
    import ast
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    need = {"model": {"ModelB_2"}, "dataset": {"ModisDatasetB", "ModisDatasetB_scale_invariance"},
            "utils": {"downscale_LST_SR_to_LR", "get_output_ftm", "model_checkpoint", "psnr_skimage", "ssim_skimage",
                      "read_JsonB", "save_model", "upsampling"}}
    src = {m: open(os.path.join(root, "dropin", m + ".py")).read() for m in need}
    for mod, names in need.items():
        tree = ast.parse(src[mod])
        defined = set()
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                defined.add(node.name)
            elif isinstance(node, ast.ImportFrom):
                defined.update((a.asname or a.name) for a in node.names)
            elif isinstance(node, ast.Assign):
                defined.update(t.id for t in node.targets if isinstance(t, ast.Name))
        assert names <= defined, (mod, names - defined)


def test_dropin_utils_host_functions(golden, tmp_path):
    """The host-only half of dropin/utils.py (no GPU): read_JsonB on a paramsB.json-shaped file (utils.py:741-764 order of
    the returned tuple), generate_psf_kernel against the reference's 9x9 kernels (golden), model_checkpoint's early-stopping
    sequence (utils.py:667-714), and the loud refusal of the out-of-scope GDAL functions."""
    import importlib
    import json
    import os
    import sys
    import numpy as np
    import pytest
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    saved = {k: sys.modules.pop(k, None) for k in ("model", "dataset", "utils")}
    sys.path.insert(0, os.path.join(root, "dropin"))
    try:
        us = importlib.import_module("utils")
        params = {"dataset_parameter": {"time": "day", "transf": "norm"},
                  "hyperparameters": {"batch_size": 8, "learning_rate": 0.001, "n_epochs": 200, "patience": 30, "alpha": 0.1, "gamma": -0.4},
                  "modelA_parameters": {"in_channels": 1}, "modelB_parameters": {"in_channels": 2, "downchannels": [16, 32, 64, 128],
                  "padding_mode": "replicate", "activation": "ReLU", "bilinear": 1, "n_bridge_blocks": 1},
                  "save_parameters": {"model_name": "modelB", "save_path": "./models/modelB_test"}, "device": "cpu"}
        f = tmp_path / "paramsB.json"
        f.write_text(json.dumps(params))
        ds, ma, mb, hy, sv, dev = us.read_JsonB(str(f))
        assert (ds, ma, mb, hy, sv, dev) == (params["dataset_parameter"], params["modelA_parameters"], params["modelB_parameters"],
                                             params["hyperparameters"], params["save_parameters"], "cpu")
        for mtf in (0.1, 0.25):
            k = us.generate_psf_kernel(1.0, 4, mtf, None)
            ref = np.array(golden["cases"][f"psf_{mtf}"]["kernel9x9"], dtype=np.float32).reshape(9, 9)
            assert k.dtype == np.float32 and np.abs(k - ref).max() < 2e-8       # outer product of the taps vs the 2-D formula
        # early stopping: improvement resets the counter; `>=` counts as no improvement; patience 2 breaks at the 2nd miss
        m = torch.nn.Linear(2, 2)
        ck = us.model_checkpoint(10, patience=2)
        metrics = {"val_loss": []}
        states = []
        for epoch, v in enumerate([1.0, 0.8, 0.8, 0.9], start=1):
            metrics["val_loss"].append(v)
            ck.test_update(m, metrics, "val_loss", epoch)
            states.append((ck.best_epoch, ck.curr_patience, ck.train_state))
        assert states == [(1, 0, None), (2, 0, "continue"), (2, 1, "continue"), (2, 2, "break")]
        assert set(ck.saved_state) == {"weight", "bias"}
        ck = us.model_checkpoint(2, patience=5)                                  # last epoch with a non-zero counter: break
        ck.test_update(m, {"val_loss": [1.0]}, "val_loss", 1)
        ck.test_update(m, {"val_loss": [1.0, 1.5]}, "val_loss", 2)
        assert ck.train_state == "break" and ck.best_epoch == 1
        # a NaN metric: the reference tests `value >= best` (False for NaN) and so treats it as an improvement -- mirrored
        ck = us.model_checkpoint(5, patience=1)
        ck.test_update(m, {"val_loss": [1.0]}, "val_loss", 1)
        ck.test_update(m, {"val_loss": [1.0, float("nan")]}, "val_loss", 2)
        assert ck.best_epoch == 2 and ck.curr_patience == 0 and ck.train_state == "continue"
        with pytest.raises(NotImplementedError, match="read_NIRRED"):
            us.read_NIRRED("x.hdf")
        # ... which is an AttributeError too, so the usual attribute protocols keep working on the overlay
        assert not hasattr(us, "read_NIRRED") and not hasattr(us, "__wrapped__") and getattr(us, "__all__", None) is None
        import inspect
        assert inspect.unwrap(us) is us
        ns = {}
        exec("from utils import *", ns)
        assert "read_JsonB" in ns and "downscale_LST_SR_to_LR" in ns
        assert us.read_JsonA(str(f))[1] == ma and len(us.read_JsonA(str(f))) == 5
        with pytest.raises(KeyError):
            us.read_JsonC(str(f))                                                # paramsB.json has no modelC_parameters, as in the reference
    finally:
        sys.path.remove(os.path.join(root, "dropin"))
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v


def test_bench_gpus_n_spawns_ranks_instead_of_exiting():
    """`python bench.py --gpus 2` (the driver's command form, no launcher environment) must START two rank processes -- a
    child `torch.distributed.run` created before the parent imports torch -- not exit with "launch with torchrun".  The
    dry-run flag lets the ranks rendezvous over gloo and sum their ranks without a GPU."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-launch"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout
    j = json.loads(line[0])
    assert j == {"dry_run": True, "world": 2, "n_gpus": 2, "rank_sum": 1.0}
    # and the parent must not have imported torch before deciding to spawn
    src = open(os.path.join(ROOT, "bench.py")).read()
    head = src[:src.index("def main()")]
    assert "\nimport torch" not in head and "\nfrom torch" not in head


def test_bench_roofline_class_selection(tmp_path):
    """bench.dominant_class() sums TotalDurationNs per kernel CLASS (all CSV rows carrying the class prefix) and returns the
    largest; the class table covers every MFMA launch of a step exactly once and its FLOPs add up to SURVEY.md §8 d."""
    import bench
    t = bench.class_table()
    launches = [lp for v in t.values() for lp in v]
    assert len(launches) == len(set(launches)) == 48 - len(bench.FUSED_BWD16)          # fused 16 -> 16 layers: one backward launch
    flops = (sum(bench.member_flops(l, p) for l, p in launches) + 2 * bench.layer_flops(0)   # the 2->16 layer has no input gradient
             + 3 * 2 * 9 * 16 * 1 * 256 * 256)                                           # outlay (16->1), three passes
    assert flops == bench.TRAIN_FLOPS_PER_PATCH
    assert sum(bench.layer_flops(l) for l, p in t["conv3x3_wgrad_wino_kernel<2, 2, true"]) * 64 == 120_795_955_200
    f = tmp_path / "x_kernel_stats.csv"
    f.write_text('"Name","Calls","TotalDurationNs"\n'
                 '"void (anonymous namespace)::conv3x3_bwd16_kernel<true>(Bwd16Args)",3,500\n'
                 '"void (anonymous namespace)::conv3x3_bwd16_kernel<false>(Bwd16Args)",1,40\n'
                 '"void (anonymous namespace)::conv3x3_wino8_kernel<4, true, true, 1>(ConvArgs)",5,300\n'
                 '"void (anonymous namespace)::conv3x3_wino8_kernel<4, true, false, 1>(ConvArgs)",1,250\n'
                 '"bn_finalize_kernel",100,9999\n')
    cls, src = bench.dominant_class(str(f))
    assert cls == "conv3x3_wino8_kernel<4, true" and src == "x_kernel_stats.csv"      # 300 + 250 > 500 + 40


def test_bench_options():
    """A plain `bench.py --gpus 1 --steps K --warmup W` times exactly K steps and leaves everything beyond the headline line to
    --full (off by default); --dump-outputs takes a directory; a run without timed steps is refused."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_bench_roofline_sources_follow_the_round_tag(tmp_path, monkeypatch):
    """Without an explicit file, bench.py --full reads the newest round's profiles, by name: a fresh checkout gives every
    committed file the same (or an arbitrary) modification time."""
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    row = '"Name","Calls","TotalDurationNs"\n"void conv3x3_%s(ConvArgs)",1,100\n'
    (prof / "r03z_kernel_stats.csv").write_text(row % "bwd16_kernel<true>")
    (prof / "r01a_kernel_stats.csv").write_text(row % "wino8_kernel<4, true, true, 1>")
    (prof / "r03z_traffic.json").write_text('{"per_launch": {"conv3x3_bwd16_kernel": {"bytes": 3}}}')
    (prof / "r01a_traffic.json").write_text('{"per_launch": {"conv3x3_bwd16_kernel": {"bytes": 1}}}')
    os.utime(prof / "r03z_kernel_stats.csv", (1, 1))
    os.utime(prof / "r03z_traffic.json", (1, 1))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.dominant_class() == ("conv3x3_bwd16_kernel", "r03z_kernel_stats.csv")
    assert bench.measured_traffic("conv3x3_bwd16_kernel") == (3, "r03z_traffic.json")


GRID_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["SIFSR_ROOT"])
from sifsr import _lib
print(_lib.call("sifsr_model_workspace_bytes", 64, 256, 256, 1))
'''


def test_bwd16_grid_knob_below_one_falls_back_to_the_default():
    """SIFSR_DBG_BWD16_GRID used to size the fused 16 -> 16 backward's persistent grid (conv3x3_bwd16_grid divided by it: 0 killed the
    process with SIGFPE, a negative value gave a launch of grid 0, so values below 1 fell back to the default).  The knob is removed:
    the grid is the constant 256 and the variable is ignored, so the workspace of the bench shape is the default one whatever it
    holds.  Each value runs in a child of its own, as when the knob was read once per process."""
    ref = _workspace_bytes_in_child("SIFSR_DBG_BWD16_GRID", None)
    assert ref > 0
    for knob in ("0", "-5"):
        assert _workspace_bytes_in_child("SIFSR_DBG_BWD16_GRID", knob) == ref, knob


def _workspace_bytes_in_child(var, value):
    """sifsr_model_workspace_bytes of the bench shape (64, 256, 256, training) in a child process with `var` = value (None: unset)."""
    import subprocess

    env = {k: v for k, v in os.environ.items() if k != var}
    env["SIFSR_ROOT"] = ROOT
    if value is not None:
        env[var] = value
    r = subprocess.run([sys.executable, "-c", GRID_WORKER], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (var, value, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
    return int(r.stdout.strip().splitlines()[-1])


def test_switch_parser_takes_any_value_and_the_workspace_covers_both_wgrad_families():
    """The one switch parser (csrc/switches.h): unset -> default, otherwise atoi.  SIFSR_WGRAD_WINO chooses between the tap-domain and
    the Winograd-domain weight-gradient kernels (1 / 2: Winograd, anything else: tap domain); the slab regions are sized for both
    families, so every value -- listed, out of range, negative, unparsable -- leaves the process alive and the workspace unchanged.
    The switches are read once per process, so each value runs in a child of its own."""
    ref = _workspace_bytes_in_child("SIFSR_WGRAD_WINO", None)
    assert ref > 0
    for value in ("0", "1", "2", "7", "-1", "x"):
        assert _workspace_bytes_in_child("SIFSR_WGRAD_WINO", value) == ref, value


REMOVED_KNOBS = ("SIFSR_DBG_CONV_GRID", "SIFSR_DBG_BWD16_GRID", "SIFSR_DBG_WGRAD_GRID_PCT", "SIFSR_DBG_WGRAD_WINO_GRID",
                 "SIFSR_DBG_WGRAD_WINO_GRID11", "SIFSR_DBG_WGRAD_WINO_GRID42", "SIFSR_DBG_WGRAD_WINO_SPLIT64", "SIFSR_DBG_WINO8_DEPTH",
                 "SIFSR_NO_WINO_WGRAD")


def test_environment_is_read_in_one_place_and_documented():
    """The library reads its run-time switches in ONE file under csrc/ (the identifier getenv occurs nowhere else), every switch name
    that file's parsing code holds as a string literal is listed in INTEGRATION.md, and the removed tuning knobs are named neither in
    csrc/ nor in INTEGRATION.md."""
    import glob
    import re

    pkg = os.path.join(ROOT, "land-surface-temperature-super-resolution-with-a-scale-invariance-free-neural-approach_amd")
    files = sorted(glob.glob(os.path.join(pkg, "csrc", "*")))
    assert len(files) > 20
    texts = {f: open(f).read() for f in files}
    readers = [f for f, t in texts.items() if re.search(r"\bgetenv\b", t)]
    assert len(readers) == 1, readers
    names = set(re.findall(r'"(SIFSR_[A-Z0-9_]+)"', texts[readers[0]]))
    assert len(names) == 10, sorted(names)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    documented = set(re.findall(r"SIFSR_[A-Z0-9_]+", doc))
    assert names <= documented, sorted(names - documented)
    # whole names: SIFSR_DBG_WGRAD_WINO_GRID is a prefix of two others
    for f, t in list(texts.items()) + [("INTEGRATION.md", doc)]:
        found = set(re.findall(r"SIFSR_[A-Z0-9_]+", t)) & set(REMOVED_KNOBS)
        assert not found, (f, sorted(found))
