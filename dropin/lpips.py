"""``from lpips import LPIPS`` (model_perf_aster_formatds.py:43, :134) on MI355X.

The reference's class downloads VGG16 (torchvision) and the linear weights (``torch.hub.load_state_dict_from_url``).  This one
never opens a URL: the two files come from the keywords ``vgg16_weights`` / ``lpips_weights`` or, without them, from the
environment variables ``SIFSR_VGG16_WEIGHTS`` / ``SIFSR_LPIPS_WEIGHTS`` -- with those set, the reference's line

    lpips_loss = LPIPS(distance = 'mse', reduction = 'mean', mean = [0.0,0.0,0.0], std = [1.0,1.0,1.0])

binds with no edit, and ``lpips_loss(t1, t2).numpy()`` (:410) works as before: CPU tensors in, a CPU float32 tensor out (device
tensors in: a device tensor out).  The max-pooling VGG16 with the squared distance is the only variant (``replace_pooling=True``
and ``distance='mae'`` raise ``NotImplementedError``)."""
import os
import sys

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import sifsr  # noqa: E402,F401
from sifsr.lpips import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from sifsr.lpips import LPIPS as _LPIPS  # noqa: E402


class LPIPS:
    def __init__(self, replace_pooling=False, distance="mse", reduction="mean", mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 vgg16_weights=None, lpips_weights=None):
        if replace_pooling:
            raise NotImplementedError("LPIPS(replace_pooling=True): only the max-pooling VGG16 runs on the device")
        if distance != "mse":
            raise NotImplementedError(f"LPIPS(distance={distance!r}): only 'mse' runs on the device")
        vgg16_weights = vgg16_weights if vgg16_weights is not None else os.environ.get("SIFSR_VGG16_WEIGHTS")
        lpips_weights = lpips_weights if lpips_weights is not None else os.environ.get("SIFSR_LPIPS_WEIGHTS")
        self._impl = _LPIPS(vgg16_weights, lpips_weights, mean=mean, std=std, reduction=reduction)
        self.reduction = reduction

    def __call__(self, x, y):
        on_host = not x.is_cuda
        dev = torch.device("cuda", torch.cuda.current_device()) if on_host else x.device
        out = self._impl(x.to(dev, torch.float32).contiguous(), y.to(dev, torch.float32).contiguous()).to(torch.float32)
        return out.cpu() if on_host else out

    forward = __call__
