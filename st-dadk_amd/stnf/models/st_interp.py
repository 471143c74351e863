"""Spatio-temporal interpolation model — MI355X build.

Drop-in for the reference's stnf/models/st_interp.py on the fixed-knot MSE path: same class
names, constructor signatures, attribute names, state_dict keys and error behaviour
(reference st_interp.py:18-150, :549-596, :599-692, :885-919), but forward()/backward() run the
hand-written HIP kernels of libstdadk.so (feature builder, fp32-MFMA MLP) whenever the tensors live on
a HIP device.  Host tensors (the reference's shipped default is `device: cpu`,
configs/config_st_interp.yaml:85) take a plain-torch statement of the same formulas further down
(`_host_*`): it exists so that the reference's driver, tests and CPU-only tooling keep working against
this package -- it is not the product's fast path, the fused engine (stnf.engine) has no host
counterpart, and nothing here touches the repository's test infrastructure.

Knot tables are generated on the host with the same torch calls the reference makes
(torch.linspace + meshgrid 'ij'), so the buffers are bit-identical by construction; only integer
index arithmetic happens on the device.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _native as N

_SCOPE_MSG = ("is not built: it needs the k_means_constrained package, which this image does not have "
              "(the reference imports it lazily in the same place, st_interp.py:362)")


_DENSE0_MAX_D = 512        # TAIL_D0_MAX of csrc/tail.h


def _round_up(a, b):
    return (a + b - 1) // b * b


def _host_phi(coords, centers, bandwidths, basis):
    """phi on host tensors with autograd: direct Euclidean distances (no matmul expansion: that form loses
    half the digits near a knot), radius = distance / (bandwidth x calibration), then the basis
    profile (reference :433-491).  coords (N,2) or (B,N,2)."""
    cal = SpatialBasisEmbedding.CALIBRATION_FACTORS[basis]
    rad = torch.cdist(coords, centers, compute_mode="donot_use_mm_for_euclid_dist") / (bandwidths * cal)
    if basis == 'wendland':
        rad = torch.clamp(rad, max=1.0)
        gap = 1.0 - rad
        gap3 = gap * gap * gap
        return gap3 * gap3 * ((35.0 * rad + 18.0) * rad + 3.0) / 3.0
    if basis == 'gaussian':
        return torch.exp(-0.5 * rad * rad)
    return torch.clamp(1.0 - rad, min=0.0)


def _host_psi(t, centers, bandwidths):
    """psi on host tensors: exp(-((t - c)/bw)^2 / 2) per temporal knot (reference :583-596)."""
    u = (t.reshape(-1, 1) - centers.reshape(1, -1)) / bandwidths.reshape(1, -1)
    return torch.exp(-0.5 * u * u)


class _PhiFunction(torch.autograd.Function):
    """phi(coords; centres, log-bandwidths) with the knot gradients of stdadk_knot_grad_f32 (module-level autograd
    of SpatialBasisEmbedding.forward, reference :433-460; no gradient flows into the coordinates)."""

    @staticmethod
    def forward(ctx, coords, centers, log_bw, basis):
        out = torch.empty(coords.shape[0], centers.shape[0], device=coords.device, dtype=torch.float32)
        N.rbf_build(coords, None, None, centers.detach().contiguous(), torch.exp(log_bw.detach()).contiguous(), basis,
                    None, None, out)
        ctx.save_for_backward(coords, centers, log_bw)
        ctx.basis = basis
        return out

    @staticmethod
    def backward(ctx, d_phi):
        coords, centers, log_bw = ctx.saved_tensors
        dc, dlb = torch.empty_like(centers, memory_format=torch.contiguous_format), torch.empty_like(log_bw)
        N.knot_grad(coords, d_phi.contiguous().float(), centers.detach().contiguous(), log_bw.detach().contiguous(),
                    ctx.basis, dc, dlb)
        return None, dc, dlb, None


class SpatialBasisEmbedding(nn.Module):
    """Multi-resolution 2-D radial basis phi(s) over fixed knot grids (reference :18-546)."""

    CALIBRATION_FACTORS = {'wendland': 1.000000, 'gaussian': 0.223477, 'triangular': 0.654714}

    def __init__(self, n_centers: list = [25, 81, 121], learnable: bool = False,
                 init_method: str = 'uniform', train_coords: np.ndarray = None,
                 basis_function: str = 'wendland', gradient_damping: bool = False,
                 damping_threshold: float = 0.3, damping_strength: float = 1.0, init_device=None,
                 init_seeding: str = 'host'):
        super().__init__()
        self.n_centers = n_centers
        self.learnable = learnable
        self.init_method = init_method
        self.basis_function = basis_function
        self.gradient_damping = gradient_damping
        self.damping_threshold = damping_threshold
        self.damping_strength = damping_strength
        if basis_function not in self.CALIBRATION_FACTORS:
            raise ValueError(f"Unknown basis function: {basis_function}. "
                             f"Choose from {list(self.CALIBRATION_FACTORS.keys())}")
        # init_seeding: where the k-means++ seeds of gmm / kmeans_balanced come from: 'host' = sklearn's kmeans_plusplus,
        # 'device' = the same random stream through stdadk_kmeanspp_f64 on init_device.  Other initialisers ignore it.
        if init_seeding not in ('host', 'device'):
            raise ValueError(f"Unknown init_seeding: {init_seeding!r}. Choose from ['host', 'device']")
        if init_seeding == 'device' and init_device is None and init_method in ('gmm', 'kmeans_balanced'):
            raise ValueError(f"init_seeding='device' needs init_device (spatial_init_device) for init_method={init_method!r}")
        if init_method == 'uniform':
            centers, bandwidths = self._init_uniform()
        elif init_method == 'gmm':
            assert train_coords is not None, "train_coords required for GMM initialization"
            # init_device: None = the host sklearn fit; a HIP device = the same mixture fitted there (stnf.knot_init)
            if init_device is None:
                centers, bandwidths = self._init_gmm(train_coords)
            else:
                from ..knot_init import gmm_knots
                centers, bandwidths = gmm_knots(train_coords, n_centers, init_device, seeding=init_seeding)
        elif init_method == 'random_site':
            assert train_coords is not None, "train_coords required for random_site initialization"
            centers, bandwidths = self._init_random_site(train_coords)
        elif init_method == 'kmeans_balanced':
            assert train_coords is not None, "train_coords required for kmeans_balanced initialization"
            # init_device: None = the reference's host path, which needs a package that is not here; a HIP device =
            # size-constrained k-means under this project's own contract (stnf.knot_init, include/stdadk.h)
            if init_device is None:
                raise NotImplementedError(f"spatial_init_method='kmeans_balanced' {_SCOPE_MSG}")
            from ..knot_init import balanced_kmeans_knots
            centers, bandwidths = balanced_kmeans_knots(train_coords, n_centers, init_device, seeding=init_seeding)
        else:
            raise ValueError(f"Unknown init_method: {init_method}")
        if learnable:
            # free centres (the training driver penalises / damps their movement), log-bandwidths as
            # the parameter so the bandwidth stays positive (reference :94-107)
            self.centers = nn.Parameter(centers)
            self.register_buffer('centers_init', centers.clone())
            self.log_bandwidths = nn.Parameter(torch.log(bandwidths))
            if gradient_damping:
                self.centers.register_hook(self._gradient_damping_hook)
        else:
            self.register_buffer('centers', centers)
            self.register_buffer('_bandwidths', bandwidths)
        self.k = centers.shape[0]
        # side length of every level (uniform grids): integer bookkeeping of the window path
        self.level_sides = [int(math.sqrt(k)) for k in n_centers]

    def _gradient_damping_hook(self, grad):
        """Scale the centres' gradient by exp(-strength * max(|c - c_init| - threshold, 0)) per knot
        (reference :111-141).  TrainStep applies the same factor inside stdadk_knot_backward_f32."""
        with torch.no_grad():
            dist = torch.norm(self.centers - self.centers_init, dim=1, keepdim=True)
            excess = torch.clamp(dist - self.damping_threshold, min=0.0)
            return grad * torch.exp(-self.damping_strength * excess)

    @property
    def bandwidths(self):
        """Positive bandwidths: exp(log_bandwidths) when learnable (reference :143-149)."""
        return torch.exp(self.log_bandwidths) if self.learnable else self._bandwidths

    def _init_uniform(self):
        """Knot table of reference :152-185: level `side x side` grid, k = ix*side + iy,
        bandwidth 2.5 x spacing, levels concatenated in list order."""
        cs, bs = [], []
        for k in self.n_centers:
            side = int(math.sqrt(k))
            assert side * side == k, f"n_centers must be perfect squares, got {k}"
            lin = torch.linspace(0, 1, side)
            gx, gy = torch.meshgrid(lin, lin, indexing='ij')
            cs.append(torch.stack([gx.flatten(), gy.flatten()], dim=-1))
            spacing = 1.0 / (side - 1) if side > 1 else 1.0
            bs.append(torch.full((k,), 2.5 * spacing))
        return torch.cat(cs, dim=0), torch.cat(bs, dim=0)

    def _grid_bandwidth(self, k):
        side = int(math.sqrt(k))
        return 2.5 * (1.0 / (side - 1) if side > 1 else 1.0)

    def _init_gmm(self, train_coords):
        """Data-adaptive knots (reference :187-264), a host-side one-off: per level a spherical
        GaussianMixture (k-means++ start, 3 restarts, 100 iterations, random_state 42) on at most
        10 000 of the training coordinates (drawn with the global numpy RNG); knots = component means,
        bandwidth = 4.23 * 2.5 * sigma, floored at a quarter of the same-size grid's bandwidth.
        Scattered knots have no grid indexing, so the model runs the materialising kernels."""
        from sklearn.mixture import GaussianMixture
        pts = np.asarray(train_coords)
        if len(pts) > 10000:
            pts = pts[np.random.choice(len(pts), 10000, replace=False)]
        pts = pts.astype(np.float64)
        cs, bs = [], []
        for k in self.n_centers:
            gm = GaussianMixture(n_components=k, covariance_type='spherical', random_state=42, max_iter=100,
                                 n_init=3, init_params='k-means++', reg_covar=1e-6, tol=1e-3, verbose=0).fit(pts)
            bw = np.clip(4.23 * 2.5 * np.sqrt(gm.covariances_), 0.25 * self._grid_bandwidth(k), float('inf'))
            cs.append(torch.from_numpy(gm.means_).float())
            bs.append(torch.from_numpy(bw).float())
        return torch.cat(cs, dim=0), torch.cat(bs, dim=0)

    def _init_random_site(self, train_coords):
        """Knots drawn from the training coordinates themselves (reference :266-343): per level k
        rows picked with the global numpy RNG (without replacement when there are enough), bandwidth
        = 2.5 x the mean distance to the (up to) 4 nearest other knots of the level."""
        from ..knot_init import neighbour_bandwidths
        pts = np.asarray(train_coords)
        cs, bs = [], []
        for k in self.n_centers:
            pick = np.random.choice(len(pts), k, replace=k > len(pts))
            c = pts[pick]
            bw = neighbour_bandwidths(c, k, self.n_centers[0])
            cs.append(torch.from_numpy(c).float())
            bs.append(torch.from_numpy(bw).float())
        return torch.cat(cs, dim=0), torch.cat(bs, dim=0)

    def forward(self, coords: torch.Tensor):
        """coords (N,2) -> phi (N,k) via stdadk_rbf_build_f32 (reference :433-460)."""
        squeeze = False
        if coords.dim() == 3:       # the reference accepts (B,N,2); flatten the batch
            b, n, _ = coords.shape
            coords, squeeze = coords.reshape(b * n, 2), (b, n)
        if not coords.is_cuda:
            out = _host_phi(coords, self.centers, self.bandwidths, self.basis_function)
            return out.view(*squeeze, self.k) if squeeze else out
        coords = coords.contiguous().float()
        if self.learnable and torch.is_grad_enabled() and (self.centers.requires_grad or self.log_bandwidths.requires_grad):
            # differentiable w.r.t. the knots, as the reference's module is (its forward is plain autograd ops)
            out = _PhiFunction.apply(coords, self.centers, self.log_bandwidths, self.basis_function)
        else:
            out = torch.empty(coords.shape[0], self.k, device=coords.device, dtype=torch.float32)
            N.rbf_build(coords, None, None, self.centers.detach(), self.bandwidths.detach(), self.basis_function,
                        None, None, out)
        return out.view(*squeeze, self.k) if squeeze else out

    def compute_domain_penalty(self, domain_bounds=(0.0, 1.0)):
        """sum of squared distances of out-of-domain centres from [lo,hi]^2 (reference :493-526)."""
        if not self.learnable:
            return torch.tensor(0.0, device=self.centers.device)
        lo, hi = domain_bounds
        viol = torch.clamp(lo - self.centers, min=0.0) + torch.clamp(self.centers - hi, min=0.0)
        return torch.sum(viol ** 2)

    def compute_movement_penalty(self):
        """sum |c - c_init|^2 (reference :528-546)."""
        if not self.learnable:
            return torch.tensor(0.0, device=self.centers.device)
        return torch.sum((self.centers - self.centers_init) ** 2)


class TemporalBasisEmbedding(nn.Module):
    """Multi-resolution 1-D Gaussian basis psi(t) (reference :549-596)."""

    def __init__(self, n_centers: list = [10, 15, 45]):
        super().__init__()
        self.n_centers = n_centers
        cs, bs = [], []
        for n in n_centers:
            cs.append(torch.linspace(0.0, 1.0, n))
            bs.append(torch.full((n,), 2.5 * (1.0 / (n - 1) if n > 1 else 1.0)))
        self.register_buffer('centers', torch.cat(cs))
        self.register_buffer('bandwidths', torch.cat(bs))
        self.k_time = self.centers.shape[0]

    def forward(self, t: torch.Tensor):
        """t (N,1) -> psi (N,k_time) via stdadk_rbf_build_f32 (reference :583-596)."""
        if not t.is_cuda:
            return _host_psi(t, self.centers, self.bandwidths)
        t = t.contiguous().float().view(-1)
        out = torch.empty(t.shape[0], self.k_time, device=t.device, dtype=torch.float32)
        N.rbf_build(None, t, None, None, None, 'wendland', self.centers, self.bandwidths, out)
        return out


class _StepFunction(torch.autograd.Function):
    """(X, coords, t) -> y_pred through libstdadk's step-level entry points; backward fills the
    parameter gradients.  No gradient flows into the inputs or the knots (fixed knots are
    buffers; reference :106-107)."""

    @staticmethod
    def forward(ctx, model, X, coords, t, training, *params):
        st = model._step_state(coords.device, force_dense=model.force_dense_path, training=training)
        B = coords.shape[0]
        y = torch.empty(B, model.output_dim, device=coords.device, dtype=torch.float32)
        ws = torch.empty(N.step_workspace_bytes(st.basis, st.desc, B, st.flags) // 4,
                         device=coords.device, dtype=torch.float32)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (training and model.dropout_p > 0) else 0
        N.forward(st.basis, st.desc, st.params, coords, t, X, B, y, ws, st.flags, training=True, seed=seed)
        ctx.model, ctx.st, ctx.seed, ctx.B = model, st, seed, B
        ctx.save_for_backward(ws, coords)
        return y

    @staticmethod
    def backward(ctx, dY):
        ws, coords = ctx.saved_tensors
        model, st = ctx.model, ctx.st
        plist = model._body_params()
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in plist]
        head = []
        if st.head is not None:
            head = [torch.empty_like(st.head[0]), torch.empty_like(st.head[1])]      # dWo, dbo
        if st.w0_transposed:
            # dW0 arrives as dW0^T (in,out); hand autograd its transpose view, shape (out,in)
            g0t = torch.empty(plist[0].shape[1], plist[0].shape[0], device=dY.device, dtype=torch.float32)
            grads[0] = g0t.t()
            gt = model._pack([g0t] + grads[1:] + head)
        else:
            gt = model._pack(grads + head)
        N.backward(st.basis, st.desc, st.params, gt, ctx.B, dY.contiguous().float(), ws, st.flags,
                   seed=ctx.seed)
        if st.head is not None:
            # d delta_l = sum_{k>=l} d beta_k; the parameter-level penalty stays with the caller's autograd
            dd = torch.empty(model.output_dim, model.last_hidden_dim + 1, device=dY.device)
            N.delta_head_backward(st.delta, head[0], head[1], 0.0, 0.0, dd)
            grads += list(dd.unbind(0))
        if model.spatial_basis.learnable:
            # plain data gradient; the damping hook on `centers` and the driver's penalty terms are
            # applied by autograd around this function, exactly as in the reference
            sb = model.spatial_basis
            dc, dlb = torch.empty_like(sb.centers), torch.empty_like(sb.log_bandwidths)
            N.knot_backward(st.basis, st.desc, st.params, coords, ctx.B, ws, st.flags, None, dc, dlb)
            grads = [dc, dlb] + grads
        return (None, None, None, None, None) + tuple(grads)


class _SparsityFunction(torch.autograd.Function):
    """(spatial, temporal) sparsity penalties of the first Linear's weight through stdadk_sparsity_f32."""

    @staticmethod
    def forward(ctx, w, p, Ks, Kt, kind, l1, lg):
        ctx.save_for_backward(w)
        ctx.cfg = (p, Ks, Kt, kind, l1, lg)
        pen = torch.zeros(2, device=w.device)
        wc = w.detach().contiguous()
        N.sparsity(N.make_sparsity(kind, l1, lg), wc, None, False, p, Ks, Kt, penalties=pen)
        return pen[0].clone(), pen[1].clone()

    @staticmethod
    def backward(ctx, gs, gt):
        (w,) = ctx.saved_tensors
        p, Ks, Kt, kind, l1, lg = ctx.cfg
        wc = w.detach().contiguous()
        dW = torch.zeros_like(wc)
        N.sparsity(N.make_sparsity(kind, l1, lg), wc, dW, False, p, Ks, Kt)      # unit gradient of both blocks
        dW[:, p:p + Ks] *= gs
        dW[:, p + Ks:p + Ks + Kt] *= gt
        return dW, None, None, None, None, None, None


class _StepState:
    """ABI descriptors for one forward/backward pair (keeps the tensors they point to alive)."""
    __slots__ = ("basis", "desc", "params", "flags", "w0_transposed", "keep", "delta", "head", "bf16")


class STInterpMLP(nn.Module):
    """[X | phi(s) | psi(t)] -> (Linear -> LayerNorm -> ReLU -> Dropout) x L -> Linear
    (reference :599-882)."""

    def __init__(self, p: int = 0, k_spatial_centers: list = [25, 81, 121],
                 k_temporal_centers: list = [10, 15, 45], hidden_dims: list = [256, 256, 128],
                 dropout: float = 0.1, layernorm: bool = True, spatial_learnable: bool = False,
                 spatial_init_method: str = 'uniform', spatial_basis_function: str = 'wendland',
                 train_coords: np.ndarray = None, gradient_damping: bool = False,
                 damping_threshold: float = 0.3, damping_strength: float = 1.0,
                 output_dim: int = 1, use_delta_reparameterization: bool = False, spatial_init_device=None,
                 spatial_init_seeding: str = 'host'):
        super().__init__()
        self.p = p
        self.k_spatial_centers = k_spatial_centers
        self.spatial_init_method = spatial_init_method
        self.spatial_basis_function = spatial_basis_function
        self.output_dim = output_dim
        self.use_delta_reparameterization = use_delta_reparameterization
        self.spatial_basis = SpatialBasisEmbedding(
            n_centers=k_spatial_centers, learnable=spatial_learnable,
            init_method=spatial_init_method, train_coords=train_coords,
            basis_function=spatial_basis_function, gradient_damping=gradient_damping,
            damping_threshold=damping_threshold, damping_strength=damping_strength,
            init_device=spatial_init_device, init_seeding=spatial_init_seeding)
        self.temporal_basis = TemporalBasisEmbedding(n_centers=k_temporal_centers)
        self.k_spatial = self.spatial_basis.k
        self.k_temporal = self.temporal_basis.k_time
        self.hidden_dims = list(hidden_dims)
        self.layernorm = bool(layernorm)
        self.dropout_p = float(dropout)

        layers, prev = [], p + self.k_spatial + self.k_temporal
        self.input_dim = prev
        for h in hidden_dims:
            layers.append(nn.Linear(prev, h))
            if layernorm:
                layers.append(nn.LayerNorm(h))
            layers.append(nn.ReLU())
            if dropout > 0:
                layers.append(nn.Dropout(dropout))
            prev = h
        self.last_hidden_dim = prev
        if use_delta_reparameterization and output_dim > 1:
            if output_dim > N.MAX_Q:
                raise NotImplementedError(f"delta head with more than {N.MAX_Q} quantiles {_SCOPE_MSG}")
            # shared trunk + one delta_k = (delta_k0 | delta_k1..d) per quantile; the output rows are
            # their cumulative sums (reference :671-686, 849-877)
            self.mlp_trunk = nn.Sequential(*layers)
            self.delta_params = nn.ParameterList([nn.Parameter(torch.zeros(prev + 1))
                                                  for _ in range(output_dim)])
            for delta_k in self.delta_params:
                nn.init.normal_(delta_k, mean=0.0, std=0.01)
        else:
            layers.append(nn.Linear(prev, self.output_dim))
            self.mlp = nn.Sequential(*layers)
            self.mlp_trunk = None
            self.delta_params = None
        # "f32" (the reference's arithmetic) or "bf16" (BASELINE config C3: the Linear layers after the first take
        # bf16 operands on the matrix cores, fp32 accumulation / LayerNorm / loss / master weights)
        self.compute_dtype = "f32"
        self._bf16_engine = None       # persistent bf16 operand copies installed by an engine (TrainStep(dtype="bf16"))
        self._bf16_refresh = None      # weak reference to that engine's refresh_bf16
        self._bf16_key = None          # identity + versions of the master weights the copies were rounded from
        # diagnostics: True forces the materialising (dense) kernels even where the window path applies
        self.force_dense_path = False
        # diagnostics: True takes the window kernels wherever supported, also for small knot tables
        self.force_window_path = False

    # ---- native plumbing ---------------------------------------------------------------
    @property
    def _has_delta(self):
        return self.delta_params is not None

    @property
    def _body(self):
        """The nn.Sequential holding the Linear/LayerNorm stack: `mlp`, or `mlp_trunk` under the delta head."""
        return self.mlp_trunk if self._has_delta else self.mlp

    def _linears(self):
        return [m for m in self._body if isinstance(m, nn.Linear)]

    def _lns(self):
        return [m for m in self._body if isinstance(m, nn.LayerNorm)]

    def _body_params(self):
        return [p for m in self._body for p in m.parameters(recurse=False)]

    def _param_list(self):
        """Parameters in registration order == order of named_parameters()."""
        sb = self.spatial_basis
        knots = [sb.centers, sb.log_bandwidths] if sb.learnable else []
        return knots + self._body_params() + (list(self.delta_params) if self._has_delta else [])

    def _bf16_copies(self, weights):
        """bf16 operand copies of the hidden Linear layers after the first (BASELINE config C3): per Linear
        index None or (W_bf16 (out,in), WT_bf16 (in,out)), rounded from `weights` (the fp32 Linear weights in
        layer order) by stdadk_bf16_shadow_refresh.  An engine (stnf.engine.TrainStep) installs persistent
        copies that its optimiser kernel keeps current; otherwise they are made afresh for the call."""
        if self._bf16_engine is not None:
            refresh = self._bf16_refresh() if self._bf16_refresh is not None else None
            if refresh is not None:
                if self._bf16_key != self._bf16_master_key():
                    refresh()              # load_state_dict / ModelEMA swap / in-place edit since the last rounding
                return self._bf16_engine
            self._bf16_engine = None       # the engine is gone: nothing keeps its copies current any more
        out = [None] * len(weights)
        n_hidden = len(self.hidden_dims)
        for l in range(1, n_hidden):
            w = weights[l]
            h, hp = w.shape
            pair = (torch.empty(h, hp, device=w.device, dtype=torch.bfloat16),
                    torch.empty(hp, h, device=w.device, dtype=torch.bfloat16))
            N.bf16_shadow_refresh(w, N.make_bf16_shadow([(0, h, hp, pair[0], pair[1])]))
            out[l] = pair
        return out

    def _bf16_master_key(self):
        """What the bf16 operand copies depend on: storage and autograd version of every hidden Linear weight after
        the first (optimizer.step(), load_state_dict and ModelEMA's copies under no_grad all bump the version) and
        the engine's own step counter (its kernels write through raw pointers and re-round in the same pass)."""
        lins = self._linears()
        return (getattr(self, "_engine_version", 0),) + tuple(
            (lins[l].weight.data_ptr(), lins[l].weight._version) for l in range(1, len(self.hidden_dims)))

    def _pack(self, flat_list, bf16=None):
        """Tensors in _body_params() order (+ the derived [Wo, bo] under the delta head) -> ABI struct."""
        it = iter(flat_list)
        Ws, bs, gs, betas = [], [], [], []
        for m in self._body:
            if isinstance(m, nn.Linear):
                Ws.append(next(it)); bs.append(next(it))
            elif isinstance(m, nn.LayerNorm):
                gs.append(next(it)); betas.append(next(it))
        if self._has_delta:
            Ws.append(next(it)); bs.append(next(it))
        return N.make_tensors(Ws, bs, gs if self.layernorm else None, betas if self.layernorm else None, bf16=bf16)

    def _delta_matrix(self, tensors=None):
        """(Q, d+1) matrix of the delta vectors (or of `tensors`, e.g. their gradients): a strided
        view when they sit equally spaced in one buffer (TrainStep's flat storage), else a stacked copy."""
        ps = [p.data for p in self.delta_params] if tensors is None else list(tensors)
        Q, d1 = len(ps), ps[0].numel()
        base = ps[0]
        stride = (ps[1].data_ptr() - base.data_ptr()) // 4 if Q > 1 else d1
        same = stride >= d1 and all(
            q.is_contiguous() and q.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
            and q.data_ptr() - base.data_ptr() == 4 * stride * k for k, q in enumerate(ps))
        if same:
            return torch.as_strided(base, (Q, d1), (stride, 1))
        return torch.stack(ps)

    def _delta_head(self, delta=None):
        """Output layer (Wo (Q,d), bo (Q,)) of the delta head: stdadk_delta_head_f32."""
        delta = self._delta_matrix() if delta is None else delta
        Wo = torch.empty(self.output_dim, self.last_hidden_dim, device=delta.device)
        bo = torch.empty(self.output_dim, device=delta.device)
        N.delta_head(delta, Wo, bo)
        return Wo, bo

    def _native_desc(self, training=True):
        return N.make_desc(self.input_dim, self.hidden_dims, self.output_dim, self.layernorm,
                           self.dropout_p if training else 0.0)

    def _native_tensors(self):
        return self._pack([p.data for p in self._body_params()] + (list(self._delta_head()) if self._has_delta else []))

    def _scattered_levels(self):
        """Level sizes for the window path over SCATTERED knots (gmm / random_site tables), or None when that path
        does not apply or would not pay: compact-support basis, at least 1024 knots, at most 8 levels, and the
        expected number of candidates per observation -- per level the knots of the cells within the largest support
        radius, (2 (ceil(reach Gk) + 1) + 1)^2 of Gk^2 cells -- at most 35 % of the table (beyond that the
        materialising kernels' dense sweep is the better program).  Taken from the bandwidths as they are now."""
        sb = self.spatial_basis
        if sb.init_method == 'uniform' or self.spatial_basis_function not in ('wendland', 'triangular'):
            return None
        if len(sb.n_centers) > 8 or self.force_dense_path:
            return None
        if self.force_window_path:                 # diagnostics / tests: the window kernels regardless of the estimate
            return list(sb.n_centers)
        if sb.k < 1024:
            return None
        cal = sb.CALIBRATION_FACTORS[self.spatial_basis_function]
        with torch.no_grad():
            bw = sb.bandwidths.detach().float().cpu()
        Gk, cand, o = N.KNOT_CELLS, 0.0, 0
        for n in sb.n_centers:
            reach = float(bw[o:o + n].max()) * cal
            o += n
            if not math.isfinite(reach):
                return None
            span = min(2 * (math.ceil(reach * Gk) + 1) + 1, Gk)
            cand += n * (span / Gk) ** 2
        return list(sb.n_centers) if cand <= 0.35 * sb.k else None

    def _basis_desc(self):
        sb, tb = self.spatial_basis, self.temporal_basis
        sides = sb.level_sides if sb.init_method == 'uniform' else self._scattered_levels()
        if sb.learnable:
            # the bandwidth slot carries log-bandwidths (FLAG_LOG_BW); knots that started as the uniform
            # grid keep their grid indexing, which lets the window path follow them as they move; scattered
            # tables are re-binned into cell lists every step
            return N.make_basis(self.p, self.spatial_basis_function, sides, sb.centers.data,
                                sb.log_bandwidths.data, tb.centers, tb.bandwidths)
        return N.make_basis(self.p, self.spatial_basis_function, sides, sb.centers, sb._bandwidths,
                            tb.centers, tb.bandwidths)

    def _step_state(self, device, force_dense=False, training=True):
        """Descriptors of the step-level ABI.  The window path wants W0 transposed (in,out):
        a TrainStep engine stores it that way (weight is then a .t() view); otherwise a transposed
        copy is made for this call when the window path applies."""
        st = _StepState()
        st.desc = self._native_desc(training)
        st.basis = self._basis_desc()
        tensors = [p.data for p in self._body_params()]
        st.delta = st.head = None
        if self._has_delta:
            st.delta = self._delta_matrix()
            st.head = self._delta_head(st.delta)        # refreshed by the owner whenever delta changes
            tensors += list(st.head)
        w0 = tensors[0]
        st.keep = None
        flags = N.FLAG_DENSE if force_dense else (N.FLAG_WINDOW if self.force_window_path else 0)
        if self.spatial_basis.learnable:
            flags |= N.FLAG_LOG_BW
        if self.spatial_basis.init_method != 'uniform' and st.basis.n_levels > 0:
            flags |= N.FLAG_SCATTERED         # the descriptor's level entries are knot counts
        if not w0.is_contiguous() and w0.t().is_contiguous():
            tensors[0] = w0.t()                                  # engine-owned (in,out) storage
            flags |= N.FLAG_W0_T
        elif (not force_dense and N.step_uses_window(st.basis, st.desc, flags | N.FLAG_W0_T)) \
                or (self.input_dim <= _DENSE0_MAX_D and len(self.hidden_dims) >= 1):
            # window path, or a feature width small enough for the library to run layer 0 inside the tail
            # launch of the materialising path: both want the first weight as (in,out)
            st.keep = w0.t().contiguous()
            tensors[0] = st.keep
            flags |= N.FLAG_W0_T
        st.bf16 = None
        if self.compute_dtype == "bf16":
            # layers after the first on the bf16 matrix cores; fp32 master weights, bf16 operand copies
            flags |= N.FLAG_BF16
            lin_w = [tensors[i] for i, p in enumerate(self._body_params()) if p.dim() == 2]
            st.bf16 = self._bf16_copies(lin_w)
        st.flags = flags
        st.w0_transposed = bool(flags & N.FLAG_W0_T)
        st.params = self._pack(tensors, bf16=st.bf16)
        return st

    def build_features(self, X, coords, t, out=None):
        """[X | phi | psi] into a row-padded (B, ld) buffer (ld multiple of 32 floats = 128 B)."""
        B = coords.shape[0]
        ld = _round_up(self.input_dim, 32)
        if out is None:
            out = torch.empty(B, ld, device=coords.device, dtype=torch.float32)
        Xc = None
        if X is not None and X.numel() > 0 and self.p > 0:
            Xc = X.contiguous().float()
        N.rbf_build(coords.contiguous().float(), t.contiguous().float().view(-1), Xc,
                    self.spatial_basis.centers.detach(), self.spatial_basis.bandwidths.detach(),
                    self.spatial_basis_function, self.temporal_basis.centers,
                    self.temporal_basis.bandwidths, out)
        return out

    # ---- reference API ------------------------------------------------------------------
    def compute_domain_penalty(self):
        return self.spatial_basis.compute_domain_penalty()

    def compute_movement_penalty(self):
        return self.spatial_basis.compute_movement_penalty()

    def get_delta_parameters(self):
        """List of the delta_k parameters, or None without the delta head (reference :712-722)."""
        if not self.use_delta_reparameterization or self.delta_params is None:
            return None
        return list(self.delta_params)

    def compute_sparsity_penalty(self, penalty_type='element', lambda_l1=0.01, lambda_group=0.01):
        """L1 / group-lasso penalties on the first layer's basis columns (reference :724-825), differentiable:
        stdadk_sparsity_f32 for value and gradient on the device.  Inside the fused engine the same kernel adds
        the gradient straight into dW0 (TrainStep(sparsity_penalty_type=...))."""
        if penalty_type not in ['element', 'group', 'sparse_group', 'none']:
            raise ValueError(f"Unknown penalty_type: {penalty_type}")
        dev = next(self.parameters()).device
        if penalty_type == 'none':
            z = torch.tensor(0.0, device=dev)
            return {'spatial_penalty': z, 'temporal_penalty': z.clone(), 'total_penalty': z.clone()}
        w = self._body[0].weight
        if w.is_cuda:
            ps, pt = _SparsityFunction.apply(w, self.p, self.k_spatial, self.k_temporal, penalty_type,
                                             float(lambda_l1), float(lambda_group))
            return {'spatial_penalty': ps, 'temporal_penalty': pt, 'total_penalty': ps + pt}
        # parameters still on the host (model not yet moved to the device): nothing for the library to do
        blocks = (w[:, self.p:self.p + self.k_spatial],
                  w[:, self.p + self.k_spatial:self.p + self.k_spatial + self.k_temporal])
        pens = []
        for blk in blocks:
            pen = torch.zeros((), device=dev)
            if penalty_type in ('group', 'sparse_group'):
                pen = pen + lambda_group * blk.norm(2, dim=0).sum()
            if penalty_type in ('element', 'sparse_group'):
                pen = pen + lambda_l1 * blk.abs().sum()
            pens.append(pen)
        return {'spatial_penalty': pens[0], 'temporal_penalty': pens[1],
                'total_penalty': pens[0] + pens[1]}

    def _host_forward(self, X, coords, t):
        """The model on host tensors, plain torch ops with autograd (`device: cpu`): [X | phi | psi] through the
        nn.Sequential stack; under the delta head the Q outputs are the trunk's features against the running sums
        of the delta vectors (intercept in slot 0), reference :849-877."""
        if next(self.parameters()).is_cuda:
            raise RuntimeError("the model's parameters are on a HIP device but the inputs are host tensors; move "
                               "the inputs (config `device: cuda`) or the model")
        cols = [self.spatial_basis(coords), self.temporal_basis(t)]
        if self.p > 0 and X is not None and X.numel() > 0:
            cols.insert(0, X)
        feats = torch.cat(cols, dim=-1)
        if not self._has_delta:
            return self.mlp(feats)
        hidden = self.mlp_trunk(feats)
        beta = torch.cumsum(torch.stack(list(self.delta_params)), dim=0)          # (Q, d+1): beta_k = sum_{l<=k} delta_l
        return hidden @ beta[:, 1:].t() + beta[:, 0]

    def forward(self, X: torch.Tensor, coords: torch.Tensor, t: torch.Tensor):
        """X (B,p), coords (B,2), t (B,1) -> y_pred (B,Q)   (reference :827-882)."""
        if not coords.is_cuda:
            return self._host_forward(X, coords, t)
        coords = coords.contiguous().float()
        t = t.contiguous().float().view(-1)
        Xc = None
        if self.p > 0:
            if X is None or X.numel() == 0:
                raise RuntimeError(f"model has p={self.p} covariates but X is empty")
            Xc = X.contiguous().float()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if need_grad:
            return _StepFunction.apply(self, Xc, coords, t, self.training, *self._param_list())
        st = self._step_state(coords.device, force_dense=self.force_dense_path, training=self.training)
        B = coords.shape[0]
        y = torch.empty(B, self.output_dim, device=coords.device, dtype=torch.float32)
        if B == 0:
            return y
        ws = torch.empty(N.step_workspace_bytes(st.basis, st.desc, B, st.flags) // 4,
                         device=coords.device, dtype=torch.float32)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (self.training and self.dropout_p > 0) else 0
        N.forward(st.basis, st.desc, st.params, coords, t, Xc, B, y, ws, st.flags,
                  training=self.training, seed=seed)
        return y


def create_model(config: dict, train_coords: np.ndarray = None) -> STInterpMLP:
    """Model from the flat config dict (reference :885-919)."""
    if config.get('regression_type', 'mean') == 'multi-quantile':
        output_dim = len(config.get('quantile_levels', [0.1, 0.5, 0.9]))
    else:
        output_dim = 1
    return STInterpMLP(
        p=config.get('p_covariates', 0),
        k_spatial_centers=config.get('k_spatial_centers', [25, 81, 121]),
        k_temporal_centers=config.get('k_temporal_centers', [10, 15, 45]),
        hidden_dims=config.get('hidden_dims', [256, 256, 128]),
        dropout=config.get('dropout', 0.1),
        layernorm=config.get('layernorm', True),
        spatial_learnable=config.get('spatial_learnable', False),
        spatial_init_method=config.get('spatial_init_method', 'uniform'),
        spatial_basis_function=config.get('spatial_basis_function', 'wendland'),
        train_coords=train_coords,
        gradient_damping=config.get('gradient_damping', False),
        damping_threshold=config.get('damping_threshold', 0.3),
        damping_strength=config.get('damping_strength', 1.0),
        output_dim=output_dim,
        use_delta_reparameterization=config.get('use_delta_reparameterization', False),
        spatial_init_device=config.get('spatial_init_device'),
        spatial_init_seeding=config.get('spatial_init_seeding', 'host'))
