"""Host-side helpers of the training driver: seeding, error metrics, the EMA shadow.  Same public names
as the reference package (its stnf/utils/__init__.py:4-14); only `grid_scores` and `basis_diagnostics` on a device
model and `field_variogram`, `grid_baselines` and `rasterize_nearest` on a HIP device reach the device library."""
from . import baselines as _baselines
from . import basis_diag as _basis_diag
from . import ema as _ema
from . import kriging as _kriging
from . import metrics as _metrics
from . import predictions as _predictions
from . import seed as _seed
from . import variogram as _variogram

set_seed = _seed.set_seed
compute_metrics = _metrics.compute_metrics
compute_spatial_metrics = _metrics.compute_spatial_metrics
print_metrics = _metrics.print_metrics
ModelEMA = _ema.ModelEMA
grid_scores = _predictions.grid_scores
save_grid_scores_npz = _predictions.save_grid_scores_npz
field_variogram = _variogram.field_variogram
variogram_curves = _variogram.variogram_curves
basis_diagnostics = _basis_diag.basis_diagnostics
save_basis_info_npz = _basis_diag.save_basis_info_npz
grid_baselines = _baselines.grid_baselines
rasterize_nearest = _baselines.rasterize_nearest
knn_host = _baselines.knn_host
knn_apply_host = _baselines.knn_apply_host
fit_variogram = _variogram.fit_variogram
kriging_weights_host = _kriging.kriging_weights_host
kriging_apply_host = _kriging.kriging_apply_host

__all__ = sorted(n for n in dir() if not n.startswith('_'))
