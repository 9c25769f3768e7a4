"""acmpc_amd - MI355X-native rollout-and-cost engine behind the ac-mpc controller's Python API.

`build_mpc` / `SpatialMPC` keep the reference's surface (src/acmpc/control/controller.py:19-29,
spatial_mpc.py:20-217); `Engine` is the thin object over the C ABI (include/acmpc.h).
"""
from ._capi import (ENSEMBLE_MAX, ENSEMBLE_MEAN, MAX_SUBSTEPS, MAX_VEHICLES, Engine, EngineError, LAYOUT_CANDIDATE_MAJOR,  # noqa: F401
                    LAYOUT_STEP_MAJOR, MODE_DYNAMIC, MODE_SPATIAL, MODE_TEMPORAL, load_library)
from .dynamic_model import DynamicBicycleParams  # noqa: F401
from .dynamic_solver import DynamicSamplingSolver  # noqa: F401
from .grip_estimator import GripEstimator  # noqa: F401
from .bicycle_model import SpatialBicycleModel  # noqa: F401
from .command_selection import TemporalCommandInterpolator, TemporalCommandSelector, steer_target  # noqa: F401
from .mpc import SpatialMPC, build_mpc  # noqa: F401
from .reference_path import ReferencePath  # noqa: F401

__all__ = ["Engine", "EngineError", "load_library", "MODE_SPATIAL", "MODE_TEMPORAL", "MODE_DYNAMIC",
           "DynamicBicycleParams", "DynamicSamplingSolver", "GripEstimator", "MAX_VEHICLES", "MAX_SUBSTEPS", "ENSEMBLE_MEAN", "ENSEMBLE_MAX",
           "LAYOUT_CANDIDATE_MAJOR",
           "LAYOUT_STEP_MAJOR", "build_mpc", "SpatialMPC", "SpatialBicycleModel", "ReferencePath",
           "TemporalCommandSelector", "TemporalCommandInterpolator", "steer_target"]
