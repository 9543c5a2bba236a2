"""mtmc_mpn -- MI355X (gfx950) native message-passing network for multi-camera tracklet association.

Import it as `mtmc_mpn` (the alias package at the repo root points here; this directory's
name is fixed by the build contract and is not a valid Python identifier).

Public surface = the reference's interface for the hot path (reference models/mpn.py, models/mlp.py):
`MOTMPNet`, `MetaLayer`, `EdgeModel`, `NodeModel`, `MLPGraphIndependent`, `MLP`, and the
`scatter_add / scatter_mean / scatter_max` functional surface of the third-party op it used.
"""
from .config import DEFAULT_ARCH, DEFAULT_GRAPH_NET_PARAMS, default_params  # noqa: F401
from .graph_build import build_graph  # noqa: F401
from .postprocess import postprocess  # noqa: F401
from . import pool  # noqa: F401
from .pool import pool_tracklets  # noqa: F401
from .grouping import Grouping, group_by_index  # noqa: F401
from . import ops  # noqa: F401
from .ops import FocalLoss, cross_entropy, cross_entropy_steps, edge_loss, focal_loss  # noqa: F401
from . import metrics  # noqa: F401
from .metrics import ClusterScores, EdgePRF, cluster_scores, edge_prf, evaluate  # noqa: F401
from .metrics import IdScores, idf1, relabel_detections  # noqa: F401
from .metrics import MotScores, mot_pairs, mot_scores, tracking_summary  # noqa: F401
from .feature_store import FeatureStore  # noqa: F401
from .modules import (MLP, EdgeModel, MetaLayer, MLPGraphIndependent, MOTMPNet,  # noqa: F401
                      NodeModel)

__all__ = ["MOTMPNet", "MetaLayer", "EdgeModel", "NodeModel", "MLPGraphIndependent", "MLP",
           "DEFAULT_GRAPH_NET_PARAMS", "DEFAULT_ARCH", "default_params", "build_graph", "postprocess", "FeatureStore", "cross_entropy", "cross_entropy_steps", "edge_loss", "ops",
           "metrics", "cluster_scores", "edge_prf", "evaluate", "ClusterScores", "EdgePRF", "pool", "pool_tracklets",
           "focal_loss", "FocalLoss", "idf1", "relabel_detections", "IdScores",
           "mot_scores", "mot_pairs", "tracking_summary", "MotScores",
           "Grouping", "group_by_index"]
