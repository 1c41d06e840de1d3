"""tissue_analysis_amd -- MI355X-native per-label voxel scan behind the SpatialImageAnalysis API.

    from tissue_analysis_amd import SpatialImageAnalysis, DICT
    analysis = SpatialImageAnalysis(labelled_volume, ignoredlabels=0, return_type=DICT, background=1)
    analysis.volume(); analysis.center_of_mass(); analysis.neighbors(); analysis.wall_areas()
    analysis.inertia_axis()

The voxel work runs in hand-written HIP kernels for gfx950 (csrc/), reached through the C ABI in
include/tissue_scan.h; there is no CPU fallback.
"""
from .spatial_image import SpatialImage
from .spatial_image_analysis import (NPLIST, LIST, DICT, AbstractSpatialImageAnalysis,
                                     SpatialImageAnalysis3D, SpatialImageAnalysis, dilation,
                                     dilation_by, real_indices, return_list_of_vectors, hollow_out_cells, wall,
                                     contact_surface, coordinates_centering3D, compute_covariance_matrix,
                                     eigen_values_vectors, distance)
from .extraction import Extraction, extract_volume
from .signal_stats import SignalStats
from .signal_quantiles import SignalHistogram, SignalQuantiles
from .signal_moments import SignalMoments
from .channel_pair import ChannelPairStats
from .cell_topology import CellTopology
from .cell_extents import CellExtents
from .cell_meshes import CellMeshes
from .label_overlap import LabelOverlap, label_overlap, lineage_from_images
from .resample import Resampled, index_matrix, transform_points
from .cell_junctions import CellJunctions, cell_junctions
from .wall_geometry import WallGeometry, wall_geometry
from .components import LabelComponents, label_components
from .distance_map import DistanceMap, distance_map
from .nearest_labels import NearestLabels
from .shell_profile import ShellProfile
from .property_graph import PropertyGraph
from .graph_from_image import graph_from_image, property_graph_to_dataframe

__all__ = ["SpatialImage", "NPLIST", "LIST", "DICT", "AbstractSpatialImageAnalysis",
           "SpatialImageAnalysis3D", "SpatialImageAnalysis", "Extraction", "extract_volume", "SignalStats", "SignalHistogram", "SignalQuantiles", "SignalMoments", "ChannelPairStats", "CellTopology", "CellExtents", "CellMeshes",
           "LabelOverlap", "label_overlap", "lineage_from_images", "Resampled", "index_matrix", "transform_points", "CellJunctions", "cell_junctions", "WallGeometry", "wall_geometry",
           "LabelComponents", "label_components", "DistanceMap", "distance_map", "NearestLabels", "ShellProfile",
           "dilation", "dilation_by", "real_indices", "return_list_of_vectors", "hollow_out_cells", "wall", "contact_surface",
           "coordinates_centering3D", "compute_covariance_matrix", "eigen_values_vectors", "distance",
           "PropertyGraph", "graph_from_image", "property_graph_to_dataframe"]
__version__ = "0.1.0"
