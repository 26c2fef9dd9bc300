"""grad_traj_optimization_amd — MI355X-native batched cost/gradient path of GTOP.

The product is the C-ABI library ``libgtop_hip.so`` (include/gtop.h) built from
csrc/ with hipcc for gfx950.  This package is the thin Python host side:
``_abi`` binds the C-ABI with ctypes, ``_lib`` wraps it (``GtopContext``), and
``problem`` generates the synthetic inputs of SURVEY.md §8d.  torch is used
only for device memory, streams and torch.distributed.

There is no CPU fallback: importing works anywhere (so the build and the
symbol check can run on a CPU box), but creating a context without a gfx950
device raises.
"""
from ._lib import (GTOP_F32, GTOP_F64, GtopError, GtopLimits, GtopParams, GtopRetime, OPTI_NODE_PARAMS,
                   GtopContext, GtopGroup, Rendezvous, box_polynomial_centres, library_path, load_library)
from .certify import (CERT_REPORT, GtopCertifyMovingOpts, GtopCertifyOpts, certify_batch, certify_device,  # noqa: F401
                      certify_moving_batch, certify_moving_device, select_best_certified_device)
from . import certify  # noqa: F401
from .insert import INSERT_INFO, GtopInsert, insert_waypoints, insert_waypoints_device  # noqa: F401
from . import insert  # noqa: F401
from .kinematics import (EXCEEDS, KIN_ABI_VERSION, KIN_ENTRY_POINTS, KIN_REPORT, KIN_SEG, UNDECIDED, WITHIN,  # noqa: F401
                         GtopKinOpts, certify_kinematics_batch, certify_kinematics_device, select_best_kin_certified_device)
from . import kinematics  # noqa: F401
from .separation import (SEP_ABI_VERSION, SEP_ENTRY_POINTS, SEP_ROW, GtopSepOpts, select_distinct_device,  # noqa: F401
                         separation_batch, separation_device, separation_workspace_bytes)
from . import separation  # noqa: F401
from .separation_certificate import (SEPCERT_ABI_VERSION, SEPCERT_ENTRY_POINTS, SEPCERT_PAIR, SEPCERT_ROW,  # noqa: F401
                                     GtopSepCertOpts, certify_separation_batch, certify_separation_device,
                                     sepcert_library, sepcert_workspace_bytes)
from . import separation_certificate  # noqa: F401
from .prediction import (PRED_ABI_VERSION, PRED_ENTRY_POINTS, PRED_INFO, GtopPredictOpts, fit_predictions,  # noqa: F401
                         fit_predictions_device, pred_abi_version, pred_library, refresh_box_predictions_device)
from . import prediction  # noqa: F401
from .timeopt import (TIME_ABI_VERSION, TIME_ENTRY_POINTS, TIME_PARTS, TIMEOPT_INFO, GtopTimeOpt,  # noqa: F401
                      optimize_times, optimize_times_device, time_abi_version, time_gradient_batch,
                      time_gradient_device, time_library)
from . import timeopt  # noqa: F401
from .timeopt_moving import (TIME_MOVING_ABI_VERSION, TIME_MOVING_ENTRY_POINTS, TIME_MOVING_PARTS,  # noqa: F401
                             optimize_times_moving, optimize_times_moving_device, time_gradient_moving_batch,
                             time_gradient_moving_device, time_moving_abi_version, time_moving_library)
from . import timeopt_moving  # noqa: F401
from .swarm import (SWARM_ABI_VERSION, SWARM_ENTRY_POINTS, GtopSwarmOpts, GtopSwarmStop, optimize_swarm,  # noqa: F401
                    optimize_swarm_device, swarm_abi_version, swarm_gradient_batch, swarm_gradient_device,
                    swarm_library, swarm_workspace_bytes)
from . import swarm  # noqa: F401
from .joint import (JOINT_ABI_VERSION, JOINT_ENTRY_POINTS, JOINT_INFO, GtopJointOpt, joint_abi_version,  # noqa: F401
                    joint_gradient_batch, joint_gradient_device, joint_library, joint_workspace_bytes, optimize_joint,
                    optimize_joint_device)
from . import joint  # noqa: F401

__all__ = ["JOINT_ABI_VERSION", "JOINT_ENTRY_POINTS", "JOINT_INFO", "GtopJointOpt", "joint", "joint_abi_version",
           "joint_gradient_batch", "joint_gradient_device", "joint_library", "joint_workspace_bytes", "optimize_joint",
           "optimize_joint_device",
           "SWARM_ABI_VERSION", "SWARM_ENTRY_POINTS", "GtopSwarmOpts", "GtopSwarmStop", "swarm", "optimize_swarm",
           "optimize_swarm_device", "swarm_abi_version", "swarm_gradient_batch", "swarm_gradient_device",
           "swarm_library", "swarm_workspace_bytes",
           "TIME_ABI_VERSION", "TIME_ENTRY_POINTS", "TIME_PARTS", "TIMEOPT_INFO", "GtopTimeOpt", "timeopt",
           "optimize_times", "optimize_times_device", "time_abi_version", "time_gradient_batch", "time_gradient_device",
           "time_library",
           "TIME_MOVING_ABI_VERSION", "TIME_MOVING_ENTRY_POINTS", "TIME_MOVING_PARTS", "timeopt_moving",
           "optimize_times_moving", "optimize_times_moving_device", "time_gradient_moving_batch",
           "time_gradient_moving_device", "time_moving_abi_version", "time_moving_library",
"PRED_ABI_VERSION", "PRED_ENTRY_POINTS", "PRED_INFO", "GtopPredictOpts", "prediction", "fit_predictions",
           "fit_predictions_device", "pred_abi_version", "pred_library", "refresh_box_predictions_device",
"SEPCERT_ABI_VERSION", "SEPCERT_ENTRY_POINTS", "SEPCERT_PAIR", "SEPCERT_ROW", "GtopSepCertOpts",
           "separation_certificate", "certify_separation_batch", "certify_separation_device", "sepcert_library",
           "sepcert_workspace_bytes",
"SEP_ABI_VERSION", "SEP_ENTRY_POINTS", "SEP_ROW", "GtopSepOpts", "separation", "select_distinct_device",
           "separation_batch", "separation_device", "separation_workspace_bytes",
"EXCEEDS", "UNDECIDED", "WITHIN", "KIN_ABI_VERSION", "KIN_ENTRY_POINTS", "KIN_REPORT", "KIN_SEG", "GtopKinOpts", "kinematics",
           "certify_kinematics_batch", "certify_kinematics_device", "select_best_kin_certified_device",
"INSERT_INFO", "GtopInsert", "insert", "insert_waypoints", "insert_waypoints_device","GTOP_F32", "GTOP_F64", "GtopError", "GtopLimits", "GtopParams", "GtopRetime", "OPTI_NODE_PARAMS",
           "GtopContext", "GtopGroup", "Rendezvous", "box_polynomial_centres", "library_path", "load_library",
           "CERT_REPORT", "GtopCertifyMovingOpts", "GtopCertifyOpts", "certify", "certify_batch", "certify_device",
           "certify_moving_batch", "certify_moving_device", "select_best_certified_device"]
