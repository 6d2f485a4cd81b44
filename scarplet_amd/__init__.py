"""scarplet_amd: MI355X-native template matching for digital elevation models.

Drop-in for the hot path of stgl/scarplet: ``match``, ``match_template``,
``compare``, ``calculate_best_fit_parameters`` and the ``WindowedTemplate``
plugin classes, with the work done by hand-written HIP kernels reached through
a C-ABI shared library (include/scarplet_hip.h).
"""

from scarplet_amd.core import (match, match_scales, match_craters, match_template, compare, load,  # noqa: F401
                               calculate_best_fit_parameters,
                               calculate_best_fit_parameters_serial, Matcher)
from scarplet_amd import WindowedTemplate, dem  # noqa: F401
from scarplet_amd.WindowedTemplate import (Scarp, Ricker, Channel, Crater,  # noqa: F401
                                           RightFacingUpperBreakScarp,
                                           LeftFacingUpperBreakScarp)
from scarplet_amd.dem import DEMGrid  # noqa: F401
from scarplet_amd.noise import estimate_curvature_noiselevel  # noqa: F401
from scarplet_amd.traces import extract_traces, Traces  # noqa: F401
from scarplet_amd.profiles import fit_profiles  # noqa: F401
from scarplet_amd.channels import fit_channels  # noqa: F401
from scarplet_amd.channel_segments import fit_channel_segments  # noqa: F401
from scarplet_amd.channel_bootstrap import bootstrap_channel_segments  # noqa: F401
from scarplet_amd.channel_strike import fit_channels_along_strike  # noqa: F401
from scarplet_amd.channel_strike_bootstrap import bootstrap_channels_along_strike  # noqa: F401
from scarplet_amd.segments import fit_segments  # noqa: F401
from scarplet_amd.bootstrap import bootstrap_segments  # noqa: F401
from scarplet_amd.strike import fit_along_strike  # noqa: F401
from scarplet_amd.strike_bootstrap import bootstrap_along_strike  # noqa: F401
from scarplet_amd.surface import snr_surface  # noqa: F401
from scarplet_amd.lateral import lateral_offsets  # noqa: F401
from scarplet_amd.plotting import plot_results, Hillshade, hillshade  # noqa: F401
from scarplet_amd._hostpool import release as release_host_buffers  # noqa: F401
