"""The model builders and what goes with them, importable from the package itself: `from ssd_keras_amd.models import build_model,
resample_classes`.  Resolved on first use, so importing a submodule (models.hdf5_lite, say) still loads nothing else."""
_EXPORTS = {"ssd_300": "keras_ssd300", "ssd_512": "keras_ssd512", "build_model": "keras_ssd7", "resample_classes": "resample"}

__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError("module {!r} has no attribute {!r}".format(__name__, name))
