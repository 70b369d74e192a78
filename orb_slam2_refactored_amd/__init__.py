"""MI355X-native ORB-SLAM2 hot path: ORB front end + local bundle adjustment on gfx950.

Host mirrors of the reference's interfaces (tiantianxuabc/ORB_SLAM2_Refactored):
  ORBextractor        <- include/ORBextractor.h
  ORBmatcher          <- include/ORBmatcher.h (Hamming kernels)
  Optimizer.LocalBundleAdjustment <- include/Optimizer.h:47
  Optimizer.PoseOptimization      <- include/Optimizer.h:49
  Optimizer.OptimizeSim3          <- src/Optimizer.cc:944-1100
  Optimizer.OptimizeEssentialGraph <- src/Optimizer.cc:743-942 (optimizer.OptimizeEssentialGraph,
                                     optimize_essential_graph_device, essential_graph_edges)
  Sim3SolverIterate               <- include/Sim3Solver.h (src/Sim3Solver.cc)
  PnPsolverIterate                <- include/PnPsolver.h (src/PnPsolver.cc); its draw table is make_pnp_draws
                                     (F, D, 4); make_draws is the Sim3 solver's (F, D, 3)
  InitializerInitialize           <- include/Initializer.h (src/Initializer.cc); its draw table is
                                     make_initializer_draws (F, T, 8)
  PreparePairs / TriangulateMatches / CreateNewMapPoints <- LocalMapping::CreateNewMapPoints
                                     (src/LocalMapping.cc:380-578), mapping.py
  KeyFrameDatabase                <- include/KeyFrameDatabase.h (src/KeyFrameDatabase.cc) and Detect's minScore
                                     (src/LoopClosing.cc:170-178), keyframe_db.py
  LocalMap                        <- LocalMap::Update and SearchLocalPoints' frustum pass (src/Tracking.cc:59-179,
                                     :554-642), local_map.py
  UpdateNormalAndDepth / UpdateConnections <- MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:341-380) and
                                     KeyFrame::UpdateConnections (src/KeyFrame.cc:94-119, 235-309), with the
                                     children and covisibility CSR exports, map_maintenance.py
  MapPointCulling / KeyFrameCulling <- LocalMapping::MapPointCulling and KeyFrameCulling (src/LocalMapping.cc:335-369,
                                     641-701) with MapPoint::SetBadFlag / EraseObservation and KeyFrame::SetBadFlag,
                                     CompactObservations and LiveChildren, culling.py
  AddKeyFrameObservations / FuseApply <- MapPoint::AddObservation and Replace (src/MapPoint.cc:109-122, 191-230) under
                                     ProcessNewKeyFrame's loop, Fuse's apply loops and CorrectLoop's matched points, with
                                     GrowObservations, observations.py
  Connected / Propagate / LoopConnections <- LoopCorrector::Correct (src/LoopClosing.cc:546-676) and the edge list of
                                     OptimizeEssentialGraph on the device, loop_correction.py
  tracking                        <- Tracking's per-frame state between the calls above (src/Tracking.cc:187-255, :490-511,
                                     :664-786, :808-814, :980-997, :1259-1313; the gather of src/Optimizer.cc:355-411):
                                     apply_matches, pose_edges, finish_pose, motion_project, end_frame, drop_outliers,
                                     stereo_points, tracking.py
  frame                           <- what System does between Extract and the Frame constructor (src/System.cc:153-219):
                                     UndistortKeyPoints, ComputeImageBounds, depth.convertTo + ComputeStereoFromRGBD and the
                                     split of cv::KeyPoint into tracking's arrays: build, build_device, frame.py
  InsertKeyFrames / CreatePoints  <- where the map grows: the KeyFrame constructor (src/KeyFrame.cc:51-64) and the MapPoint
                                     constructor with AddObservation / AddMapPoint / Map::AddMapPoint (src/MapPoint.cc:44-56,
                                     src/Tracking.cc:724-736, :981-997, :1104-1126, src/LocalMapping.cc:562-575) on the slot
                                     tables, with the slot allocation, creation.py
All compute runs in liborbslam2_amd.so (HIP kernels behind include/orbslam2_amd.h).
"""
from .extractor import ORBextractor, KP_DTYPE
from .matcher import (ORBmatcher, ComputeStereoMatches, Fuse, fuse_device, SearchByProjectionSim3,
                      search_by_projection_sim3_device, SearchBySim3, search_by_sim3_device,
                      ComputeDistinctiveDescriptors, compute_distinctive_descriptors_device)
from . import optimizer
from . import tracking
from . import frame
from .sim3solver import Sim3SolverIterate, sim3solver_iterate_device, make_draws
from .pnpsolver import PnPsolverIterate, pnpsolver_iterate_device, make_draws as make_pnp_draws
from .initializer import InitializerInitialize, initializer_initialize_device, make_draws as make_initializer_draws
from .mapping import (PreparePairs, TriangulateMatches, CreateNewMapPoints, prepare_pairs_device,
                      triangulate_matches_device, create_new_map_points_device)
from .keyframe_db import KeyFrameDatabase
from .local_map import LocalMap
from .map_maintenance import (UpdateNormalAndDepth, update_normal_depth_device, UpdateConnections,
                              update_connections_device, Children, children_device, CovisCsr, covis_csr_device)
from .culling import (MapPointCulling, map_point_culling_device, KeyFrameCulling, keyframe_culling_device,
                      CompactObservations, compact_observations_device, LiveChildren, live_children_device)
from .observations import (AddKeyFrameObservations, add_keyframe_observations_device, FuseApply, fuse_apply_device,
                           GrowObservations, grow_observations_device)
from .creation import InsertKeyFrames, insert_keyframes_device, CreatePoints, create_points_device
from .synth import synth_image, shifted_pair, stereo_pair, make_pose_batch

__all__ = ["InsertKeyFrames", "insert_keyframes_device", "CreatePoints", "create_points_device", "AddKeyFrameObservations", "add_keyframe_observations_device", "FuseApply", "fuse_apply_device", "GrowObservations",
           "grow_observations_device", "MapPointCulling", "map_point_culling_device", "KeyFrameCulling", "keyframe_culling_device", "CompactObservations",
           "compact_observations_device", "LiveChildren", "live_children_device", "KeyFrameDatabase", "LocalMap", "UpdateNormalAndDepth", "update_normal_depth_device", "UpdateConnections",
           "update_connections_device", "Children", "children_device", "CovisCsr", "covis_csr_device", "PreparePairs", "TriangulateMatches", "CreateNewMapPoints", "prepare_pairs_device", "triangulate_matches_device",
           "create_new_map_points_device", "InitializerInitialize", "initializer_initialize_device", "make_initializer_draws", "PnPsolverIterate", "pnpsolver_iterate_device", "make_pnp_draws", "Sim3SolverIterate", "sim3solver_iterate_device", "make_draws", "ORBextractor", "ORBmatcher", "ComputeStereoMatches", "Fuse", "fuse_device", "SearchByProjectionSim3",
           "search_by_projection_sim3_device", "SearchBySim3", "search_by_sim3_device", "ComputeDistinctiveDescriptors",
           "compute_distinctive_descriptors_device", "optimizer", "KP_DTYPE", "synth_image", "shifted_pair", "stereo_pair",
           "make_pose_batch", "tracking", "frame"]
