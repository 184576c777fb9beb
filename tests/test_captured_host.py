"""CPU: the captured step and the captured granule predictors at any ratio -- what can be held without a GPU.

  * the refusals that are reached before any launch: the untrainable pair (20, 24) with the rule named, a non-capturable optimizer,
    `valid` without `masked` (and the reverse), bad `kind`, `batch`, `conserve`, a geometry `ratio.geometry` refuses, a step that
    does not belong to the epoch loop's model / optimizer / factor;
  * the new options are keyword-only and ADDED AROUND the calls (`_granule.keyword_options`, as `conserve.granule_option`): the
    positional signatures the older host tests pin are what they were;
  * f23 adds no kernel and no C-ABI entry point: `_lib.FAMILIES` has its 18 rows and include/ holds the same 18 headers.

There is nothing numerical here: every comparison of tests/test_captured_gpu.py is for equal bits."""
import inspect
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = {"mean_lst": 300.0, "std_lst": 10.0, "mean_ndvi": 0.4, "std_ndvi": 0.3}
HEADERS = ["sifsr_adapt.h", "sifsr_baselines.h", "sifsr_conserve.h", "sifsr_degrade.h", "sifsr_dms.h", "sifsr_gaps.h", "sifsr_hip.h",
           "sifsr_lpips.h", "sifsr_masked.h", "sifsr_mosaic.h", "sifsr_products.h", "sifsr_ratio.h", "sifsr_rconserve.h", "sifsr_rloss.h",
           "sifsr_rproducts.h", "sifsr_scores.h", "sifsr_sensor.h", "sifsr_spectra.h"]


def cpu_model_and_optimizer(capturable=True):
    import sifsr
    m = sifsr.ModelB_2(2)
    return m, sifsr.FlatAdam(m.parameters(), lr=1e-3, capturable=capturable)


class NoLaunch(torch.nn.Module):
    """a model whose parameters nobody may ask for: a refusal that reaches it came too late"""

    def parameters(self, recurse=True):
        raise AssertionError("the constructor went on after a refusal")

    def forward(self, x):
        raise AssertionError("a forward ran")


# ---- 1. rloss.GraphedTrainStep -------------------------------------------------------------------------------------------------------
def test_graphed_train_step_refusals():
    import sifsr
    from sifsr import rloss
    E = sifsr.SifsrError
    m, opt = cpu_model_and_optimizer()
    with pytest.raises(E, match=r"\(20, 24\) is not a trainable pair.*sensor\.lr_shape"):             # the rule is named
        rloss.GraphedTrainStep(NoLaunch(), opt, 2, STATS, 0.5, 1.0, 20, 24)
    with pytest.raises(E, match="ratio.geometry refuses"):
        rloss.GraphedTrainStep(NoLaunch(), opt, 2, STATS, 0.5, 1.0, 8, 20)                            # hr is no multiple of 8
    with pytest.raises(E, match="kind"):
        rloss.GraphedTrainStep(NoLaunch(), opt, 2, STATS, 0.5, 1.0, 8, 24, kind="sr3")
    for bad in (0, -1):
        with pytest.raises(E, match="batch"):
            rloss.GraphedTrainStep(NoLaunch(), opt, bad, STATS, 0.5, 1.0, 8, 24)
    with pytest.raises(ValueError, match="capturable=True"):
        rloss.GraphedTrainStep(NoLaunch(), cpu_model_and_optimizer(False)[1], 2, STATS, 0.5, 1.0, 8, 24)
    # the call: valid goes with masked, and only with it -- refused before anything is copied or launched
    lst, up, v = torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 24, 24), torch.ones(2, 1, 8, 8, dtype=torch.uint8)
    c = torch.tensor([128, 1152])
    plain = rloss.GraphedTrainStep(m, opt, 2, STATS, 0.5, 1.0, 8, 24)
    masked = rloss.GraphedTrainStep(m, opt, 2, STATS, 0.5, 1.0, 8, 24, masked=True, return_sr=True)
    assert plain.valid is None and plain.counts is None and plain.factor == 3.0 and plain.batch == 2
    assert tuple(masked.valid.shape) == (2, 1, 8, 8) and masked.valid.dtype == torch.uint8
    assert tuple(masked.counts.shape) == (2,) and masked.counts.dtype == torch.int64
    assert tuple(masked.lst.shape) == (2, 1, 8, 8) and tuple(masked.lst_up.shape) == tuple(masked.ndvi.shape) == (2, 1, 24, 24)
    for step, kw in ((plain, dict(valid=v)), (plain, dict(counts=c)), (plain, dict(valid=v, counts=c)), (masked, {}), (masked, dict(counts=c))):
        with pytest.raises(ValueError, match="masked=True"):
            step(lst, up, up, **kw)
    with pytest.raises(ValueError, match="counts"):
        masked(lst, up, up, valid=v, counts=torch.zeros(3, dtype=torch.int64))
    for step in (plain, masked):
        assert step.graph is None and step._warm == 0 and not step.lst.any()                          # nothing ran, nothing was copied


def test_epoch_loops_check_the_step_before_the_first_batch():
    from sifsr import rloss

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader was read after a refusal")

    m, opt = cpu_model_and_optimizer()
    other_m, other_opt = cpu_model_and_optimizer()
    step = rloss.GraphedTrainStep(m, opt, 2, STATS, 0.5, 1.0, 8, 24)
    with_sr = rloss.GraphedTrainStep(m, opt, 2, STATS, 0.5, 1.0, 8, 24, return_sr=True)
    epoch = lambda **kw: rloss.train_epoch(kw.pop("model", m), Loader(), kw.pop("optimizer", opt), STATS, 0.5, 1.0, kw.pop("factor", 3.0),
                                           device="cpu", **kw)
    with pytest.raises(ValueError, match="return_sr=True"):
        epoch(graphed=step)                                                                           # metrics are on by default
    for kw in (dict(model=other_m), dict(optimizer=other_opt), dict(factor=2.5), dict(kind="sr1")):
        with pytest.raises(ValueError, match="another model, optimizer, kind or factor"):
            epoch(graphed=with_sr, **kw)
    with pytest.raises(ValueError, match="rloss.GraphedTrainStep"):
        epoch(graphed=object())
    with pytest.raises(ValueError, match="return_sr=True"):
        rloss.fit(m, Loader(), Loader(), 1, opt, STATS, 0.5, 1.0, 3.0, graphed=step)


# ---- 2. the granule predictors -------------------------------------------------------------------------------------------------------
def test_ratio_granule_predictor_refusals():
    import sifsr
    from sifsr import ratio
    E = sifsr.SifsrError
    G = lambda *a, **kw: ratio.GranulePredictor(NoLaunch(), *a, **kw)
    assert ratio.geometry((20, 28), 8, 24, 2, True).tiles == (3, 5)                                   # the layout of the GPU tests exists
    for shape, kw in (((20, 28), dict(window=8, hr=20)),                   # hr no multiple of 8
                      ((21, 28), dict(window=16, hr=40)),                  # a side that is no multiple of q = 2
                      ((36, 50), dict(window=16, hr=40, overlap=3)),       # an overlap that is no multiple of q
                      ((20, 28), dict(window=8, hr=24, overlap=5)),        # 2 overlap > window
                      ((4, 28), dict(window=8, hr=24)),                    # smaller than a window
                      ((20, 28), dict(window=65, hr=192)),
                      ("20x28", dict(window=8, hr=24))):
        with pytest.raises(E, match="tile layout|geometry"):
            G(shape, STATS, **kw)
    for kw, what in ((dict(batch=0), "batch"), (dict(batch=-3), "batch"), (dict(conserve=-1), "conserve"), (dict(conserve=65), "conserve")):
        with pytest.raises(E, match=what):
            G((20, 28), STATS, window=8, hr=24, **kw)
    with pytest.raises(E, match="multiple of 4"):                                                   # the tile selection's rule, gaps only
        G((18, 30), STATS, window=6, hr=24, gaps=True)
    sig = [(k, v.default) for k, v in inspect.signature(ratio.GranulePredictor.__init__).parameters.items()][1:]
    E_ = inspect.Parameter.empty
    assert sig[:-2] + sig[-1:] == [("model", E_), ("lst_shape", E_), ("stats", E_), ("window", 64), ("hr", 192), ("overlap", 0),
                                   ("cover_edges", False), ("batch", 256), ("conserve", 0), ("gaps", False), ("device", None)]
    assert sig[-2][0] == "fill_value" and math.isnan(sig[-2][1])


def test_x4_granule_predictor_refusals_and_signature():
    import sifsr
    from sifsr import predict
    E = sifsr.SifsrError
    G = lambda *a, **kw: predict.GranulePredictor(NoLaunch(), *a, **kw)
    for kw, what in ((dict(batch=0), "batch"), (dict(conserve=-1), "conserve"), (dict(window=6), "multiple of 4"),
                     (dict(batch=0, gaps=True), "batch"), (dict(conserve=-1, gaps=True), "conserve"), (dict(window=6, gaps=True), "multiple of 4")):
        with pytest.raises(E, match=what):
            G((20, 28), STATS, **dict(dict(window=8, overlap=2, cover_edges=True), **kw))
    with pytest.raises(TypeError):
        G((20, 28), STATS, 8, 2, True, 4, None, 0, True)                                              # gaps is keyword-only
    # the positional signature is what it was; the options are on the wrapper, keyword-only in effect, off by default
    assert list(inspect.signature(predict.GranulePredictor.__init__).parameters) == ["self", "model", "lst_shape", "stats", "window", "overlap",
                                                                                     "cover_edges", "batch", "device", "conserve"]
    assert "cannot have a data-dependent batch count" not in " ".join(predict.GranulePredictor.__doc__.split())
    assert "fixed slot count and a device-side active count" in " ".join(predict.GranulePredictor.__doc__.split())


# ---- 3. the options of the loops -----------------------------------------------------------------------------------------------------
def test_options_are_added_around_the_calls():
    from sifsr import _granule, adapt, rloss
    for f, option, default in ((rloss.train_epoch, "graphed", None), (rloss.fit, "graphed", None), (rloss.adapt_granule, "graphed", False)):
        assert option not in inspect.signature(f).parameters and option in f.__doc__
        outer = inspect.signature(f, follow_wrapped=False).parameters
        assert [p.kind for p in outer.values()] == [inspect.Parameter.VAR_POSITIONAL, inspect.Parameter.VAR_KEYWORD]
        with pytest.raises(TypeError):
            f(graphed=default, no_such_option=1)
    p = inspect.signature(adapt.adapt_granule).parameters
    assert list(p)[-2:] == ["optimizer", "graphed"] and p["graphed"].default is False
    # the decorator itself: options are taken out, the rest is bound to the stated signature, defaults applied
    seen = []

    def impl(a, b, c, extra="x"):
        seen.append((a, b, c, extra))
        return a + b + c

    @_granule.keyword_options(impl, extra="x")
    def f(a, b=2, c=3):
        """doc"""

    assert f(1) == 6 and f(1, c=5, extra="y") == 8 and seen == [(1, 2, 3, "x"), (1, 2, 5, "y")]
    assert f.__doc__ == "doc" and list(inspect.signature(f).parameters) == ["a", "b", "c"]
    with pytest.raises(TypeError):
        f(1, 2, 3, 4)
    with pytest.raises(TypeError):
        f()


def test_adapt_granule_graphed_needs_a_capturable_optimizer():
    """refused before the first launch: CPU rasters would raise SifsrError at `fill_gaps`, the first one"""
    import sifsr
    from sifsr import _granule, adapt
    m, opt = cpu_model_and_optimizer(False)
    lay = _granule.Layout(8, 24, 2, True, (3, 5), (60, 84), None, None, None, None)
    with pytest.raises(ValueError, match="capturable=True"):
        adapt._adapt(m, lay, None, torch.zeros(20, 28), torch.zeros(60, 84), STATS, None, 5, 4, 1e-3, opt, captured=lambda *a: None)
    with pytest.raises(sifsr.SifsrError):                                                           # a capturable one passes that check
        adapt._adapt(m, lay, None, torch.zeros(20, 28), torch.zeros(60, 84), STATS, None, 5, 4, 1e-3, cpu_model_and_optimizer()[1],
                     captured=lambda *a: None)


# ---- 4. no kernel, no entry point, no family -----------------------------------------------------------------------------------------
def test_the_table_and_the_headers_are_what_they_were():
    import sifsr
    from sifsr import _lib
    assert len(_lib.FAMILIES) == 18
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == HEADERS
    assert sorted(os.path.basename(_lib.header_path(f)) for f in _lib.FAMILIES) == HEADERS
    for name in ("GraphedTrainStep",):
        assert hasattr(sifsr.rloss, name) and hasattr(sifsr.train, name) and getattr(sifsr.rloss, name) is not getattr(sifsr.train, name)
    assert sifsr.ratio.GranulePredictor is not sifsr.predict.GranulePredictor
    assert issubclass(sifsr.ratio.GranulePredictor, sifsr._granule.CapturedGranule)
    assert issubclass(sifsr.predict.GranulePredictor, sifsr._granule.CapturedGranule)
    for text in (sifsr.ratio.__doc__, sifsr.rloss.__doc__, sifsr.__doc__):
        assert "f23" in text
