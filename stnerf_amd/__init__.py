"""Importable alias for the ``st-nerf_amd/`` package directory.

The product tree lives in ``st-nerf_amd/`` (the name the build contract fixes); a hyphen is not importable, so this package
puts that directory first on its ``__path__`` -- ``import stnerf_amd.<x>`` then resolves to ``st-nerf_amd/<x>`` through the
normal import machinery (no ``exec``) -- and re-exports what ``st-nerf_amd/__init__.py`` defines (docstring, version).
"""
import importlib.util as _util
import os as _os

_pkg = _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "st-nerf_amd")
if not _os.path.isdir(_pkg):
    raise ImportError(f"{_pkg} is missing: the stnerf_amd alias must sit beside the st-nerf_amd/ package directory")
__path__.insert(0, _pkg)
_spec = _util.spec_from_file_location(__name__ + "._package_init", _os.path.join(_pkg, "__init__.py"))
_init = _util.module_from_spec(_spec)
_spec.loader.exec_module(_init)
__doc__ = _init.__doc__
__version__ = _init.__version__


def __getattr__(name):
    # (lazily: importing the alias package alone stays free of torch)
    if name == "BackgroundCache":
        from stnerf_amd.bkgd_cache import BackgroundCache
        return BackgroundCache
    if name == "LayerCache":
        from stnerf_amd.layer_cache import LayerCache
        return LayerCache
    if name == "OccupancyGrids":
        from stnerf_amd.occupancy import OccupancyGrids
        return OccupancyGrids
    if name == "ProposalGrids":
        from stnerf_amd.proposal import ProposalGrids
        return ProposalGrids
    if name == "Termination":
        from stnerf_amd.termination import Termination
        return Termination
    if name == "AccumulateSpec":
        from stnerf_amd.accumulate import AccumulateSpec
        return AccumulateSpec
    if name == "LatticeSpec":
        from stnerf_amd.lattice import LatticeSpec
        return LatticeSpec
    if name == "Lens":
        from stnerf_amd.lens import Lens
        return Lens
    if name in ("ReprojectSpec", "BackgroundPlate"):
        from stnerf_amd import reproject
        return getattr(reproject, name)
    if name in ("DeepSpec", "DeepFrame"):
        from stnerf_amd import deep
        return getattr(deep, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
