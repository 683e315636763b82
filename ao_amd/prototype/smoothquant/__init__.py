"""SmoothQuant (torchao/prototype/smoothquant): SmoothQuantConfig through quantize_, and its observers."""
from .api import SmoothQuantConfig, SmoothQuantStep
from .core import RunningAbsMaxSmoothQuantObserver, SmoothQuantObservedLinear, SmoothQuantObserver

__all__ = ["SmoothQuantConfig", "SmoothQuantStep", "SmoothQuantObserver", "RunningAbsMaxSmoothQuantObserver", "SmoothQuantObservedLinear"]
