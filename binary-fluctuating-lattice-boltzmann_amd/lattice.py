"""Host-side mirror of the reference's LBM operator surface (LBM_binary.H) for one z-slab.

The method names, argument meaning and state semantics follow the reference's free
functions so that tests read like the reference's own driver (main_run_job.cpp:269-339):

    LBM_init_mixture / LBM_init_stripe(frac) / LBM_init_droplet(r) / LBM_init(f0, g0)
    LBM_timestep()                       LBM_binary.H:545-594
    LBM_hydrovars_density() -> hydrovsbar  :343-354
    thermal_noise() -> fnoisevs, gnoisevs  :73-132
    LBM_hydrovars() -> hydrovs             :298-313
    update_com()                           LBM_hydrovs.H:26-60

All arithmetic happens in the HIP library behind the C-ABI (include/bflbm.h); this file
only moves numpy arrays in AMReX FAB layout (component slowest, x fastest) across it.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import Domain, Fab, Params, NVEL, NHYDRO, NHYDROBAR, check


def default_params(**overrides):
    """The reference's shipped globals (LBM_binary.H:17-30, LBM_d3q19.H:6-10)."""
    p = Params()
    _lib.load().bflbm_default_params(ctypes.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown model parameter {k!r}")
        setattr(p, k, v)
    return p


def make_fab(lo, hi, vlo=None, vhi=None):
    """bflbm_fab for a host array allocated over cells lo..hi with valid region vlo..vhi."""
    f = Fab()
    vlo = lo if vlo is None else vlo
    vhi = hi if vhi is None else vhi
    for d in range(3):
        f.lo[d], f.hi[d], f.vlo[d], f.vhi[d] = int(lo[d]), int(hi[d]), int(vlo[d]), int(vhi[d])
    return f


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _check_array(a, ncomp, shape3, name):
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous:
        raise TypeError(f"{name}: need a C-contiguous float64 numpy array")
    if a.shape != (ncomp,) + tuple(shape3):
        raise ValueError(f"{name}: shape {a.shape}, expected {(ncomp,) + tuple(shape3)}")


class _DevicePlane:
    """A component plane of the resident state as seen by torch.as_tensor (no copy)."""

    def __init__(self, ptr, ndoubles):
        self.__cuda_array_interface__ = {"shape": (int(ndoubles),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}


class _DropletMixin:
    """Droplet observables reduced on the device (csrc/bflbm_droplet.h); `_droplet_fn` names the C-ABI pair."""

    def droplet_moments(self):
        """20 raw mass moments of rho (see include/bflbm.h); feed analysis.*_from_moments."""
        m = (ctypes.c_double * 20)()
        check(getattr(self.lib, self._droplet_fn[0])(self._h, m))
        return np.array(list(m))

    def fit_droplet(self, r0=None, p0=None, max_iter=200, tol=1e-12):
        """(hi, lo, R, W) of the tanh profile about r0 (default: the centre of mass), unit-box coordinates.
        Start values default to the notebook's (max rho, min rho, 0.5, 0.5) with max/min replaced by the
        model's natural bounds rho_hi, rho_lo of the parameters."""
        from . import analysis
        if r0 is None:
            r0 = analysis.com_from_moments(self.droplet_moments(), self.n)
        if p0 is None:
            p0 = (float(self.params.rho_hi), float(self.params.rho_lo), 0.5, 0.5)
        r = (ctypes.c_double * 3)(*[float(v) for v in r0])
        p = (ctypes.c_double * 4)(*[float(v) for v in p0])
        cost, it = ctypes.c_double(), ctypes.c_int()
        check(getattr(self.lib, self._droplet_fn[1])(self._h, r, p, int(max_iter), float(tol), ctypes.byref(cost), ctypes.byref(it)))
        self.last_fit = dict(cost=cost.value, iterations=it.value)
        return tuple(p)

    def fit_droplet_flow(self, **opts):
        """(W, R, undulation) of the reference's own gradient-flow fit (fittingDropletParams, LBM_hydrovs.H:160-213):
        rho ~ 1/2 (1 + tanh((R - |r - r0|) / sqrt(2 W))) in unit-box coordinates.  Keyword options are the fields of
        bflbm_flowfit_opts (W0, R0, eta_W, eta_R, dt, undul_ratio, nstep, step_window, max_retry); the driver's call is
        fit_droplet_flow(step_window=20, undul_ratio=0.01, nstep=400, W0=kappa, R0=radius) (main_run_job.cpp:365).
        Raises BflbmError where the reference throws (undulation out of bounds after the retries)."""
        o = _lib.FlowFitOpts()
        self.lib.bflbm_flowfit_default_opts(ctypes.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise AttributeError(f"unknown fit option {k!r}")
            setattr(o, k, v)
        res = (ctypes.c_double * 3)()
        retries = ctypes.c_int()
        check(getattr(self.lib, self._droplet_fn[2])(self._h, ctypes.byref(o), res, ctypes.byref(retries)))
        self.last_fit = dict(retries=retries.value)
        return tuple(res)


def _register(owner, dep):
    """`dep` lives on `owner`: owner.close() meets it first (closes it, or calls its _owner_closing where it has one)."""
    if not hasattr(owner, "_dependents"):
        owner._dependents = []
    owner._dependents.append(dep)


def _unregister(owner, dep):
    deps = getattr(owner, "_dependents", [])
    if dep in deps:
        deps.remove(dep)


class _Recorder:
    """What Trace and InterfaceTrace share: the handle made by `create` on the owner, closed before the owner it reads,
    and the calls <_abi>_destroy / _sample / _reset / _count."""

    def __init__(self, owner, create, *args):
        self.lib, self.owner = owner.lib, owner
        h = ctypes.c_void_p()
        check(getattr(self.lib, create)(owner._h, *args, ctypes.byref(h)))
        self._h = h
        _register(owner, self)

    def _call(self, name, *args):
        return getattr(self.lib, self._abi + "_" + name)(self._h, *args)

    def close(self):
        if getattr(self, "_h", None):
            self._call("destroy")
            self._h = None
            _unregister(self.owner, self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample(self):
        """Record the resident state now (e.g. frame 0); the every-counter does not move."""
        check(self._call("sample"))

    def reset(self):
        """Forget the samples and restart the every-counter."""
        check(self._call("reset"))

    def _count(self):
        n, b = ctypes.c_longlong(), ctypes.c_int()
        check(self._call("count", ctypes.byref(n), ctypes.byref(b)))
        return n.value, b.value

    @property
    def count(self):
        return self._count()[0]

    _geometry_types = (ctypes.c_int,) * 4

    def _geometry(self):
        """The numbers of <_abi>_geometry: every kind's geometry() says what they are."""
        v = [t() for t in self._geometry_types]
        check(self._call("geometry", *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _window(self, first=0, count=None):
        """(first, count, B, steps[count, B] int64 to fill) of a read of the samples first ... first + count - 1
        (count None: all from `first`)."""
        n, b = self._count()
        count = n - int(first) if count is None else int(count)
        return int(first), count, b, np.empty((max(count, 0), b), dtype=np.int64)


class Trace(_Recorder):
    """Droplet moments of every replica recorded on the device every `every` steps through the owner (a lone
    single-slab BinaryLBM, a BatchLBM or a RingLBM) and read once: include/bflbm.h, "Ensemble traces".  Made by owner.trace()."""
    _abi = "bflbm_trace"

    def __init__(self, owner, create, every, capacity, threshold):
        super().__init__(owner, create, int(every), int(capacity), -np.inf if threshold is None else float(threshold))

    def read(self):
        """(steps[count, B] int64, rec[count, B, 12]); synchronises the owner's stream."""
        _, n, b, steps = self._window()
        rec = np.empty((n, b, _lib.TRACE_NREC))
        check(self.lib.bflbm_trace_read(self._h, 0, n, _ptr(rec), _ptr(steps)))
        return steps, rec

    def com(self):
        """Centre of mass [count, B, 3] in cell indices of the cells above the threshold."""
        rec = self.read()[1]
        return rec[..., 1:4] / rec[..., 0:1]


IFACE_FIELDS = {"rho": 0, "phi": 1}


class InterfaceTrace(_Recorder):
    """Contour heights of every column of every replica recorded on the device every `every` steps through the owner (a
    lone single-slab BinaryLBM or a BatchLBM) and read once: include/bflbm.h, "Interface traces".  Made by
    owner.interface_trace(); an owner may carry several."""
    _abi = "bflbm_iface"

    def __init__(self, owner, create, level, field, window, every, capacity):
        if field not in IFACE_FIELDS and field not in IFACE_FIELDS.values():
            raise ValueError(f"interface_trace: field {field!r}, expected 'rho' (0) or 'phi' (1)")
        z_lo, z_hi = (0, owner.n[2]) if window is None else (int(window[0]), int(window[1]))
        super().__init__(owner, create, int(IFACE_FIELDS.get(field, field)), float(level), z_lo, z_hi, int(every), int(capacity))
        self.level, self.field, self.window = float(level), field, (z_lo, z_hi)

    def geometry(self):
        """(nx, ny, segments of the scan, pairs (z-1, z) per segment): which launch shape the library chose."""
        return self._geometry()

    def read(self):
        """(steps[count, B] int64, h[count, B, 2, ny, nx]), direction 0 rising, 1 falling, NaN where a column has no
        crossing; synchronises the owner's stream."""
        _, n, b, steps = self._window()
        nx, ny = self.geometry()[:2]
        h = np.empty((n, b, 2, ny, nx))
        check(self.lib.bflbm_iface_read(self._h, 0, n, _ptr(h), _ptr(steps)))
        return steps, h

    def rising(self):
        """h[count, B, ny, nx] of the first pair with d(z-1) < level <= d(z)."""
        return self.read()[1][:, :, 0]

    def falling(self):
        """h[count, B, ny, nx] of the first pair with d(z-1) >= level > d(z)."""
        return self.read()[1][:, :, 1]


class ShapeTrace(_Recorder):
    """Droplet radii along fixed rays from a centre, for every replica, recorded on the device every `every` steps through
    the owner (a lone single-slab BinaryLBM or a BatchLBM) and read once: include/bflbm.h, "Shape traces".  The device
    stand-in for the marching-cubes surface and its spherical-harmonic expansion of Droplet_Fluctuation.ipynb (cells 32,
    38, 41).  Made by owner.shape_trace(); an owner may carry several."""
    _abi = "bflbm_shape"

    def __init__(self, owner, create, level, nodes, field, direction, centre, threshold, step, rmax, every, capacity):
        from . import analysis
        if field not in IFACE_FIELDS and field not in IFACE_FIELDS.values():
            raise ValueError(f"shape_trace: field {field!r}, expected 'rho' (0) or 'phi' (1)")
        if direction not in analysis.SHAPE_DIRECTIONS and direction not in analysis.SHAPE_DIRECTIONS.values():
            raise ValueError(f"shape_trace: direction {direction!r}, expected 'falling' (0) or 'rising' (1)")
        dirs, weights = analysis.ray_nodes(16, 32) if nodes is None else nodes
        self.dirs = np.ascontiguousarray(dirs, dtype=np.float64)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        if self.dirs.ndim != 2 or self.dirs.shape[1] != 3 or self.weights.shape != (len(self.dirs),):
            raise ValueError(f"shape_trace: nodes = (dirs[ndir, 3], weights[ndir]), got shapes {self.dirs.shape} and {self.weights.shape}")
        rmax = min(owner.n) / 2 if rmax is None else float(rmax)
        step = float(step)
        if not (np.isfinite(step) and step > 0 and np.isfinite(rmax)):
            raise ValueError(f"shape_trace: step {step} must be finite and > 0, rmax {rmax} finite")
        nsteps = int(np.floor(rmax / step))
        c = None if centre is None else (ctypes.c_double * 3)(*[float(v) for v in centre])
        thr = -np.inf if threshold is None else float(threshold)
        super().__init__(owner, create, int(IFACE_FIELDS.get(field, field)), float(level),
                         int(analysis.SHAPE_DIRECTIONS.get(direction, direction)), c, thr, len(self.dirs),
                         self.dirs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), step, nsteps, int(every), int(capacity))
        self.level, self.field, self.direction, self.step = float(level), field, direction, step

    def geometry(self):
        """(ndir, nsteps, segments of the ray kernel, pairs (k-1, k) per segment): which launch shape the library chose."""
        return self._geometry()

    def read(self):
        """(steps[count, B] int64, centre[count, B, 3], r[count, B, ndir]): the centre used (cell indices x, y, z) and the
        radius along every ray, NaN where a ray has no crossing; synchronises the owner's stream."""
        _, n, b, steps = self._window()
        ndir = self.geometry()[0]
        rec = np.empty((n, b, 3 + ndir))
        check(self.lib.bflbm_shape_read(self._h, 0, n, _ptr(rec), _ptr(steps)))
        return steps, rec[..., :3], rec[..., 3:]

    def modes(self, lmax):
        """a[count, B, (lmax + 1)^2] = analysis.shape_modes of the recorded radii on the trace's nodes: the zeta_lm(t) of
        the notebook's cells 38 and 41; NaN for a frame with a ray without a crossing."""
        from . import analysis
        return analysis.shape_modes(self.read()[2], self.dirs, self.weights, lmax)


FSTAT_SOURCES = {"hydrovs": 0, "hydrovsbar": 1, "noise": 2}


def fstat_variable_names(source):
    """The component names of a field-statistics source: plotfile.variable_names for hydrovs (22) and hydrovsbar (9),
    WriteOutNoise's fa0 .. fa18, ga0 .. ga18 for the noise moments.  FieldStats also takes fn<k> / gn<k> for fa<k> / ga<k>
    and "rhot" for component 5 (rho + phi, the equilibrium_rhot field, which VariableNames calls p_bulk)."""
    from . import plotfile
    if source == 2:
        return plotfile.noise_names("f") + plotfile.noise_names("g")
    return plotfile.variable_names(NHYDROBAR if source == 1 else NHYDRO)


def _ints(values):
    """A ctypes int array of the values, of one entry at least: the library refuses a null pointer."""
    values = list(values)
    return (ctypes.c_int * max(len(values), 1))(*values)


class _FieldRecorder(_Recorder):
    """What the recorders that read observed fields share (csrc/bflbm_fieldsel.h is the library's side of it): a source,
    variables of it by name or component index, pairs of recorded variables by name or slot, and an owner whose close()
    detaches the recorder, which stays readable until its own close().  `_label` starts the kind's ValueErrors,
    `_nsources` is how many of FSTAT_SOURCES the kind takes."""
    _label, _nsources = None, 2

    def _owner_closing(self):
        """The owner's close(): the library detaches the recorder; what it recorded stays readable until close()."""
        _unregister(self.owner, self)

    def _select(self, source, variables, pairs=()):
        """Sets source, component_names, variables (component indices) and pairs (of slots; a lone name: with itself) and
        returns them as the library takes them: (nvars, vars, npairs, pair_a, pair_b)."""
        accepted = {k: v for k, v in FSTAT_SOURCES.items() if v < self._nsources}
        if source not in accepted and source not in accepted.values():
            expected = f"one of {sorted(accepted)} or 0..2" if self._nsources == 3 else "'hydrovs' (0) or 'hydrovsbar' (1)"
            raise ValueError(f"{self._label}: source {source!r}, expected {expected}")
        self.source = int(accepted.get(source, source))
        self.component_names = fstat_variable_names(self.source)
        items = [variables] if isinstance(variables, (str, int, np.integer)) else list(variables)
        self.variables = [self._component(v) for v in items]
        self.pairs = [(self._slot(a), self._slot(b)) for a, b in [(p, p) if isinstance(p, str) else p for p in pairs]]
        return (len(self.variables), _ints(self.variables), len(self.pairs),
                _ints(p[0] for p in self.pairs), _ints(p[1] for p in self.pairs))

    def _alias(self, name):
        """A kind's own names: the component name they stand for, or the component index."""
        return name

    def _component(self, v):
        """A variable by name or by component index of the source."""
        v = self._alias(v) if isinstance(v, str) else int(v)
        if not isinstance(v, str):
            return v
        if v not in self.component_names:
            raise ValueError(f"{self._label}: variable {v!r}, expected one of {self.component_names} or an index")
        return self.component_names.index(v)

    def _slot(self, v):
        """A recorded variable by name or by slot (its position in the variable list)."""
        if not isinstance(v, str):
            return int(v)
        c = self._component(v)
        if c not in self.variables:
            raise ValueError(f"{self._label}: {v!r} is not one of the recorded variables")
        return self.variables.index(c)

    def _recorded_names(self):
        """The recorded variables by name, in slot order."""
        return [self.component_names[c] if 0 <= c < len(self.component_names) else str(c) for c in self.variables]


class SpectrumTrace(_FieldRecorder):
    """The structure factor of chosen pairs of hydrodynamic variables of every sample, binned into shells in |q| or into
    |k| along one axis, recorded on the device every `every` steps through the owner (a lone single-slab BinaryLBM, a
    BatchLBM or a RingLBM) and read once: include/bflbm.h, "Spectrum traces".  Made by owner.spectrum_trace(); an owner may carry
    several.  Closing the owner detaches the trace: it stays readable until its own close()."""
    _abi = "bflbm_spectrum"
    _geometry_types = (ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int)

    def __init__(self, owner, create, names_or_pairs, kind, every, capacity, lb_hydrovars, zero_avg, var_scaling):
        from . import analysis, structfact
        if isinstance(kind, str) and kind not in analysis.SPECTRUM_KINDS:
            raise ValueError(f"spectrum_trace: kind {kind!r}, expected one of {sorted(analysis.SPECTRUM_KINDS)} or 0..3")
        items = list(names_or_pairs)
        if items and isinstance(items[0], str):              # variable names: the pairs of structfact.StructFact
            self.names = items
            self.pairs = structfact.StructFact(items).pairs
        else:
            self.names = None
            self.pairs = [(int(a), int(b)) for a, b in items]
        n = len(self.pairs)
        self.scale = [1.0] * n if var_scaling is None else [float(v) for v in var_scaling]
        if len(self.scale) != n:
            raise ValueError(f"spectrum_trace: {len(self.scale)} scalings for {n} pairs")
        self.kind, self.lb, self.zero_avg = int(analysis.SPECTRUM_KINDS.get(kind, kind)), bool(lb_hydrovars), bool(zero_avg)
        sc = (ctypes.c_double * max(n, 1))(*self.scale)
        super().__init__(owner, create, n, _ints(p[0] for p in self.pairs), _ints(p[1] for p in self.pairs), sc, int(self.lb), self.kind, int(self.zero_avg), int(every), int(capacity))

    def pair_names(self):
        names = self.names
        if names is None:
            from . import plotfile
            names = plotfile.variable_names(NHYDROBAR if self.lb else NHYDRO)
        return ["struct_fact_%s_%s" % (names[b], names[a]) for a, b in self.pairs]

    def geometry(self):
        """(bins, pairs, chunks of the sorted index list, the most chunks any bin has): what the library built."""
        return self._geometry()

    def bins(self):
        """(count[nbins] int64: full-spectrum modes per bin, q[nbins]: the bin's wave number)."""
        nbins = self.geometry()[0]
        count, q = np.empty(nbins, dtype=np.int64), np.empty(nbins)
        check(self.lib.bflbm_spectrum_bins(self._h, _ptr(count), _ptr(q)))
        return count, q

    def read(self):
        """(steps[count, B] int64, sums[count, B, npairs, nbins]); synchronises the owner's stream."""
        _, n, b, steps = self._window()
        nbins, npairs = self.geometry()[:2]
        sums = np.empty((n, b, npairs, nbins))
        check(self.lib.bflbm_spectrum_read(self._h, 0, n, _ptr(sums), _ptr(steps)))
        return steps, sums

    def mean(self):
        """sums / count [count, B, npairs, nbins]: the bin averages, NaN where a bin has no modes."""
        count = self.bins()[0]
        sums = self.read()[1]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(count > 0, sums / count, np.nan)


class ModeTrace(_FieldRecorder):
    """The complex Fourier amplitudes of chosen hydrodynamic variables at chosen integer wavevectors, for every replica,
    recorded on the device every `every` steps through the owner (a lone single-slab BinaryLBM or a BatchLBM) and read
    once: include/bflbm.h, "Mode traces".  What time correlations are made of (analysis.time_correlation).  Made by
    owner.mode_trace(); an owner may carry several.  Closing the owner detaches the trace: it stays readable until its
    own close()."""
    _abi, _label = "bflbm_modes", "mode_trace"

    def __init__(self, owner, create, variables, modes, every, capacity, lb_hydrovars):
        self.lb = bool(lb_hydrovars)
        nv, va = self._select(int(self.lb), variables)[:2]
        m = np.asarray(modes)
        if m.ndim != 2 or m.shape[1] != 3 or not np.issubdtype(m.dtype, np.integer):
            raise ValueError(f"mode_trace: modes is an integer array [nmodes, 3], got shape {m.shape} of {m.dtype}")
        self.modes = np.ascontiguousarray(m, dtype=np.int32)
        nm = len(self.modes)
        super().__init__(owner, create, nv, va, int(self.lb), nm, self.modes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                         int(every), int(capacity))

    def geometry(self):
        """(variables, wavevectors, tiles per plane, sites per tile): what the library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(steps[count, B] int64, amp[count, B, nvars, nmodes] complex128) of the samples first ... first + count - 1
        (count None: all from `first`); synchronises the owner's stream."""
        first, count, b, steps = self._window(first, count)
        nv, nm = self.geometry()[:2]
        amp = np.empty((max(count, 0), b, nv, nm), dtype=np.complex128)
        check(self.lib.bflbm_modes_read(self._h, first, count, _ptr(amp), _ptr(steps)))
        return steps, amp


FSTAT_WHAT = {"sum": 0, "mean": 1, "first": 2, "prod": 3, "cov": 4}


class FieldStats(_FieldRecorder):
    """The running mean of chosen fields at every site over the frames taken, and chosen second moments around it,
    accumulated on the device for a lone single-slab BinaryLBM, every replica of a BatchLBM or a RingLBM:
    include/bflbm.h, "Field statistics"; analysis.field_statistics is the same arithmetic in numpy.  Made by
    owner.field_stats().  every = 0: fed by sample() only.  An owner may carry several.  Closing the owner detaches the
    recorder: it stays readable until its own close()."""
    _abi, _label, _nsources = "bflbm_fstat", "field_stats", 3

    def __init__(self, owner, create, variables, pairs, source, every):
        selection = self._select(source, variables, pairs)   # a lone name among the pairs: its variance
        self.names = self.component_names                    # every component of the source
        super().__init__(owner, create, self.source, *selection, int(every))
        self.shape = (owner.n[2], owner.n[1], owner.n[0])

    def _alias(self, name):
        if self.source == 2 and len(name) > 2 and name[:2] in ("fn", "gn") and name[2:].isdigit():
            return name[0] + "a" + name[2:]
        if self.source != 2 and name == "rhot":            # component 5, rho + phi, which VariableNames calls p_bulk
            return 5
        return name

    def _pair(self, p):
        """A recorded pair by index or as (a, b) of names or slots."""
        if isinstance(p, (int, np.integer)):
            return int(p)
        p = (p, p) if isinstance(p, str) else p
        key = (self._slot(p[0]), self._slot(p[1]))
        if key not in self.pairs:
            raise ValueError(f"field_stats: the pair {p!r} is not recorded")
        return self.pairs.index(key)

    def _get(self, what, index, replica):
        out = np.empty(self.shape)
        check(self.lib.bflbm_fstat_get(self._h, FSTAT_WHAT[what], int(index), int(replica), _ptr(out)))
        return out

    def mean(self, v, replica=0):
        """sum * (1 / N) of a variable (name or slot) [nz, ny, nx]; replica -1: the ensemble mean.  Synchronises."""
        return self._get("mean", self._slot(v), replica)

    def cov(self, p, replica=0):
        """The covariance (divisor N) of a pair (index, or (a, b) of names or slots) [nz, ny, nx]; replica -1: the mean
        within-replica covariance.  Synchronises."""
        return self._get("cov", self._pair(p), replica)

    def sum(self, v, replica=0):
        return self._get("sum", self._slot(v), replica)

    def first(self, v, replica=0):
        return self._get("first", self._slot(v), replica)

    def prod(self, p, replica=0):
        return self._get("prod", self._pair(p), replica)


PROFILE_AXES = {"x": 0, "y": 1, "z": 2}


class ProfileTrace(_FieldRecorder):
    """The sums of chosen hydrovs / hydrovsbar variables, and of chosen products of them, over every lattice plane normal
    to one axis, for every replica, recorded on the device every `every` steps through the owner (a lone single-slab
    BinaryLBM, a BatchLBM or a RingLBM) and read once: include/bflbm.h, "Profile traces"; analysis.plane_profiles is the
    same arithmetic in numpy, analysis.pressure_profile turns the means into the pressure profile.  Made by
    owner.profile_trace(); an owner may carry several.  Closing the owner detaches the trace: it stays readable until its
    own close()."""
    _abi, _label = "bflbm_profile", "profile_trace"

    def __init__(self, owner, create, variables, pairs, axis, source, every, capacity):
        selection = self._select(source, variables, pairs)   # a lone name among the pairs: its square
        if axis not in PROFILE_AXES and axis not in PROFILE_AXES.values():
            raise ValueError(f"profile_trace: axis {axis!r}, expected one of {sorted(PROFILE_AXES)} or 0..2")
        self.axis = int(PROFILE_AXES.get(axis, axis))
        super().__init__(owner, create, self.source, self.axis, *selection, int(every), int(capacity))
        self.plane_sites = owner.n[0] * owner.n[1] * owner.n[2] // owner.n[self.axis]

    names = property(_FieldRecorder._recorded_names, doc="The recorded variables by name, in slot order: what analysis.pressure_profile takes.")

    def geometry(self):
        """(Q = variables + pairs, planes along the axis, sites of a work item, partials per (q, plane)): what the
        library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(sums[count, B, Q, n_a], steps[count, B] int64) of the samples first ... first + count - 1 (count None: all
        from `first`); the variables first, then the pairs; synchronises the owner's stream."""
        first, count, b, steps = self._window(first, count)
        nq, na = self.geometry()[:2]
        sums = np.empty((max(count, 0), b, nq, na))
        check(self.lib.bflbm_profile_read(self._h, first, count, _ptr(sums), steps.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return sums, steps

    def means(self, first=0, count=None):
        """sums / (sites of a plane) [count, B, Q, n_a]: the plane averages."""
        return self.read(first, count)[0] / float(self.plane_sites)


class HistogramTrace(_FieldRecorder):
    """The counts of the sites of chosen hydrovs / hydrovsbar / noise variables over fixed bins, and of chosen pairs of
    them over the product of two binnings, for every replica, recorded on the device as 64-bit integers every `every`
    steps through the owner (a lone single-slab BinaryLBM, a BatchLBM or a RingLBM; the noise source not on a batch) and
    read once: include/bflbm.h, "Histogram traces"; analysis.field_histograms is the same rule in numpy.  `ranges` is
    {variable: (lo, hi, nbins)} with the names of fstat_variable_names (or component indices) in recording order, `pairs`
    a list of (a, b) of recorded variables by name or slot.  Made by owner.histogram_trace(); an owner may carry several.
    Closing the owner detaches the trace: it stays readable until its own close()."""
    _abi, _label, _nsources = "bflbm_hist", "histogram_trace", 3
    _alias = FieldStats._alias

    def __init__(self, owner, create, ranges, pairs, source, every, capacity):
        items = list(ranges.items()) if hasattr(ranges, "items") else [(v, r) for v, *r in ranges]
        if any(len(r) != 3 for _, r in items):
            raise ValueError("histogram_trace: ranges = {variable: (lo, hi, nbins)}")
        selection = self._select(source, [v for v, _ in items], [tuple(p) for p in pairs])
        self.lo = np.array([float(r[0]) for _, r in items], dtype=np.float64)
        self.hi = np.array([float(r[1]) for _, r in items], dtype=np.float64)
        self.nbins = [int(r[2]) for _, r in items]
        nv, va, npairs, pa, pb = selection
        lo, hi = (self.lo, self.hi) if nv else (np.zeros(1), np.ones(1))
        super().__init__(owner, create, self.source, nv, va, _ptr(lo), _ptr(hi), _ints(self.nbins), npairs, pa, pb, int(every), int(capacity))
        self.sites = owner.n[0] * owner.n[1] * owner.n[2]

    names = property(_FieldRecorder._recorded_names, doc="The recorded variables by name, in slot order.")

    def geometry(self):
        """(C, [(offset, length) of every block: the variables, then the pairs], sites of a work item, workgroups per
        replica of the counting launch, 32-bit LDS counters of a workgroup): what the library built."""
        scalars = [ctypes.c_int() for _ in range(5)]
        off, length = (ctypes.c_int * 12)(), (ctypes.c_int * 12)()
        c, nb, tile, groups, lds = [ctypes.byref(x) for x in scalars]
        check(self._call("geometry", c, nb, off, length, tile, groups, lds))
        nblocks = scalars[1].value
        return (scalars[0].value, [(off[k], length[k]) for k in range(nblocks)]) + tuple(x.value for x in scalars[2:])

    def _block(self, k):
        return self.geometry()[1][k]

    def _pair(self, p):
        """A recorded pair by index or as (a, b) of names or slots."""
        if isinstance(p, (int, np.integer)):
            return int(p)
        key = (self._slot(p[0]), self._slot(p[1]))
        if key not in self.pairs:
            raise ValueError(f"histogram_trace: the pair {p!r} is not recorded")
        return self.pairs.index(key)

    def read(self, first=0, count=None):
        """(steps[count, B] int64, counts[count, B, C] int64) of the samples first ... first + count - 1 (count None: all
        from `first`); synchronises the owner's stream."""
        first, count, b, steps = self._window(first, count)
        counts = np.empty((max(count, 0), b, self.geometry()[0]), dtype=np.int64)
        as_ll = ctypes.POINTER(ctypes.c_longlong)
        check(self.lib.bflbm_hist_read(self._h, first, count, counts.ctypes.data_as(as_ll), steps.ctypes.data_as(as_ll)))
        return steps, counts

    def hist(self, v):
        """The bins of a variable (name or slot) [count, B, nbins_v]."""
        off, n = self._block(self._slot(v))
        return self.read()[1][..., off:off + n - 3]

    def outliers(self, v):
        """(below, above, nan) of a variable [count, B, 3]."""
        off, n = self._block(self._slot(v))
        return self.read()[1][..., off + n - 3:off + n]

    def joint(self, p):
        """(cells[count, B, na, nb], outside[count, B]) of a pair (index, or (a, b) of names or slots)."""
        p = self._pair(p)
        off, n = self._block(len(self.variables) + p)
        rec = self.read()[1]
        na, nb = self.nbins[self.pairs[p][0]], self.nbins[self.pairs[p][1]]
        return rec[..., off:off + n - 1].reshape(rec.shape[:2] + (na, nb)), rec[..., off + n - 1]

    def edges(self, v):
        """The nbins_v + 1 bin edges lo + k (hi - lo) / nbins of a variable, for plotting: membership is by the rule of
        include/bflbm.h, which these reproduce up to rounding."""
        s = self._slot(v)
        return self.lo[s] + (self.hi[s] - self.lo[s]) * np.arange(self.nbins[s] + 1) / self.nbins[s]

    def pdf(self, v):
        """The in-range counts divided by (in-range count x bin width) [count, B, nbins_v]; NaN where no site is in range."""
        s = self._slot(v)
        h = self.hist(s).astype(np.float64)
        width = (self.hi[s] - self.lo[s]) / self.nbins[s]
        with np.errstate(invalid="ignore", divide="ignore"):
            return h / (h.sum(axis=-1, keepdims=True) * width)


MORPH_SIDES = {"above": 0, "below": 1}


class MorphologyTrace(_FieldRecorder):
    """The Minkowski functionals of the set {v >= level} (side "above") or {v < level} (side "below") of one hydrovs /
    hydrovsbar variable at 1 to 8 levels, for every replica, recorded on the device as 64-bit integer counts of cubes,
    faces, edges and vertices every `every` steps through the owner (a lone single-slab BinaryLBM or a BatchLBM; no
    rings) and read once: include/bflbm.h, "Morphology traces"; analysis.minkowski_counts is the same rule in numpy.
    Made by owner.morphology_trace(); an owner may carry several (rho and phi, or both sides).  Closing the owner
    detaches the trace: it stays readable until its own close()."""
    _abi, _label = "bflbm_morph", "morphology_trace"
    _geometry_types = (ctypes.c_int,) * 5
    _alias = FieldStats._alias

    def __init__(self, owner, create, variable, levels, side, source, every, capacity):
        if side not in MORPH_SIDES and side not in MORPH_SIDES.values():
            raise ValueError(f"morphology_trace: side {side!r}, expected 'above' (0) or 'below' (1)")
        if not isinstance(variable, (str, int, np.integer)):
            raise ValueError(f"morphology_trace: one variable by name or component index, got {variable!r}")
        self._select(source, variable)
        self.side = int(MORPH_SIDES.get(side, side))
        self.levels = np.atleast_1d(np.asarray(levels, dtype=np.float64)).copy()
        if self.levels.ndim != 1:
            raise ValueError(f"morphology_trace: levels is a number or a list of 1..8 numbers, got shape {self.levels.shape}")
        lv = self.levels if len(self.levels) else np.zeros(1)
        super().__init__(owner, create, self.source, self.variables[0], len(self.levels), _ptr(lv), self.side, int(every), int(capacity))
        self.sites = owner.n[0] * owner.n[1] * owner.n[2]

    names = property(_FieldRecorder._recorded_names, doc="The recorded variable by name, a list of one.")

    def geometry(self):
        """(levels, plane sites of a work item's tile, its planes Zc, work items per replica, workgroups of the counting
        launch over all replicas): what the library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(steps[count, B] int64, counts[count, B, nlevels, 4] int64: N3, N2, N1, N0, the cubes, faces, edges and
        vertices) of the samples first ... first + count - 1 (count None: all from `first`); synchronises the owner's
        stream."""
        first, count, b, steps = self._window(first, count)
        counts = np.empty((max(count, 0), b, len(self.levels), 4), dtype=np.int64)
        as_ll = ctypes.POINTER(ctypes.c_longlong)
        check(self.lib.bflbm_morph_read(self._h, first, count, counts.ctypes.data_as(as_ll), steps.ctypes.data_as(as_ll)))
        return steps, counts

    def functionals(self, first=0, count=None):
        """[count, B, nlevels, 4] int64: V, S, 2B, chi (analysis.minkowski_functionals of the counts)."""
        from . import analysis
        return analysis.minkowski_functionals(self.read(first, count)[1])

    def length(self, first=0, count=None):
        """[count, B, nlevels]: the real-space domain size nsites / S (analysis.morphology_length), NaN where S = 0."""
        from . import analysis
        return analysis.morphology_length(self.read(first, count)[1], self.sites)


class ChordTrace(_FieldRecorder):
    """The chord-length distributions along x, y and z of the set {v >= level} (side "above") or {v < level} (side
    "below") of one hydrovs / hydrovsbar variable at 1 to 8 levels, for every replica, recorded on the device as 64-bit
    integers every `every` steps through the owner (a lone single-slab BinaryLBM or a BatchLBM; no rings) and read once:
    include/bflbm.h, "Chord traces"; analysis.chord_counts is the same rule in numpy, analysis.chord_blocks the layout.
    A chord is a maximal run of occupied sites along a periodic line; runs of max_length sites and more share the last
    bin.  Made by owner.chord_trace(); an owner may carry several (rho and phi, or both sides).  Closing the owner
    detaches the trace: it stays readable until its own close()."""
    _abi, _label = "bflbm_chord", "chord_trace"
    _geometry_types = (ctypes.c_int,) * 7
    _alias = FieldStats._alias

    def __init__(self, owner, create, variable, levels, side, max_length, source, every, capacity):
        if side not in MORPH_SIDES and side not in MORPH_SIDES.values():
            raise ValueError(f"chord_trace: side {side!r}, expected 'above' (0) or 'below' (1)")
        if not isinstance(variable, (str, int, np.integer)):
            raise ValueError(f"chord_trace: one variable by name or component index, got {variable!r}")
        self._select(source, variable)
        self.side = int(MORPH_SIDES.get(side, side))
        self.levels = np.atleast_1d(np.asarray(levels, dtype=np.float64)).copy()
        if self.levels.ndim != 1:
            raise ValueError(f"chord_trace: levels is a number or a list of 1..8 numbers, got shape {self.levels.shape}")
        lv = self.levels if len(self.levels) else np.zeros(1)
        self.max_length = int(max_length)
        super().__init__(owner, create, self.source, self.variables[0], len(self.levels), _ptr(lv), self.side, self.max_length, int(every), int(capacity))
        self.n = tuple(owner.n)
        self.sites = owner.n[0] * owner.n[1] * owner.n[2]
        self.words = 1 + 3 * (3 + self.max_length)

    names = property(_FieldRecorder._recorded_names, doc="The recorded variable by name, a list of one.")

    def geometry(self):
        """(levels, max_length M, words W of a level, 32-bit LDS counters of a workgroup, workgroups of the x, the y and
        the z launch over all replicas): what the library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(steps[count, B] int64, counts[count, B, nlevels, W] int64: the occupied sites, then per axis x, y, z the
        chords, the spanning lines, long_sites and h[1..M]) of the samples first ... first + count - 1 (count None: all
        from `first`); synchronises the owner's stream."""
        first, count, b, steps = self._window(first, count)
        counts = np.empty((max(count, 0), b, len(self.levels), self.words), dtype=np.int64)
        as_ll = ctypes.POINTER(ctypes.c_longlong)
        check(self.lib.bflbm_chord_read(self._h, first, count, counts.ctypes.data_as(as_ll), steps.ctypes.data_as(as_ll)))
        return steps, counts

    def _word(self, axis, what, first, count):
        from . import analysis
        return self.read(first, count)[1][..., analysis.chord_blocks(self.max_length)[analysis._chord_axis(axis)][what]]

    def occupied(self, first=0, count=None):
        """[count, B, nlevels] int64: the occupied sites V."""
        return self.read(first, count)[1][..., 0]

    def chords(self, axis, first=0, count=None):
        """[count, B, nlevels] int64: the chords along an axis ("x", "y", "z" or 0..2)."""
        return self._word(axis, "chords", first, count)

    def spanning(self, axis, first=0, count=None):
        """[count, B, nlevels] int64: the fully occupied lines along an axis, which carry no chord."""
        return self._word(axis, "spanning", first, count)

    def hist(self, axis, first=0, count=None):
        """[count, B, nlevels, M] int64: h[1..M] along an axis, the last bin holding the chords of M sites and more."""
        return self._word(axis, "hist", first, count)

    def mean_length(self, axis, first=0, count=None):
        """[count, B, nlevels]: the mean chord (V - n_a spanning) / chords along an axis (analysis.chord_mean_length),
        NaN where there is no chord."""
        from . import analysis
        return analysis.chord_mean_length(self.read(first, count)[1], self.n)[..., "xyz".index(analysis._chord_axis(axis))]

    def pdf(self, axis, first=0, count=None):
        """[count, B, nlevels, M]: h / chords along an axis, the fraction of the chords per bin (width 1; the last bin
        is open-ended); NaN where there is no chord."""
        h = self.hist(axis, first, count).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return h / h.sum(axis=-1, keepdims=True)


class CoarseTrace(_FieldRecorder):
    """The sums of chosen hydrovs / hydrovsbar variables, and of chosen products of them, over the blocks of a periodic
    window of the box, for every replica, recorded on the device every `every` steps through the owner (a lone
    single-slab BinaryLBM or a BatchLBM; no rings) and read once: include/bflbm.h, "Coarse traces"; analysis.coarse_fields
    is the same arithmetic in numpy.  With block (1, 1, 1) a sample is a slice or a sub-volume, with a larger block a
    coarse movie.  origin, extent and block are (x, y, z); extent None: from the origin to the end of the box.  Made by
    owner.coarse_trace(); an owner may carry several.  Closing the owner detaches the trace: it stays readable until its
    own close()."""
    _abi, _label = "bflbm_coarse", "coarse_trace"
    _geometry_types = (ctypes.c_int,) * 7

    def __init__(self, owner, create, variables, pairs, block, origin, extent, source, every, capacity):
        selection = self._select(source, variables, pairs)   # a lone name among the pairs: its square
        self.origin = self._triple("origin", origin)
        self.extent = tuple(n - o for n, o in zip(owner.n, self.origin)) if extent is None else self._triple("extent", extent)
        self.block = self._triple("block", block)
        super().__init__(owner, create, self.source, *selection, _ints(self.origin), _ints(self.extent), _ints(self.block), int(every), int(capacity))
        self.block_sites = self.block[0] * self.block[1] * self.block[2]

    @staticmethod
    def _triple(what, v):
        try:
            t = tuple(int(x) for x in v)
        except TypeError:
            t = ()
        if len(t) != 3:
            raise ValueError(f"coarse_trace: {what} is three integers (x, y, z), got {v!r}")
        return t

    names = property(_FieldRecorder._recorded_names, doc="The recorded variables by name, in slot order.")

    @property
    def sum_names(self):
        """The Q sums by name: the variables, then "a*b" for every pair."""
        names = self.names
        return names + [f"{names[a]}*{names[b]}" for a, b in self.pairs]

    def geometry(self):
        """(c_x, c_y, c_z, Q = variables + pairs, fine sites of an x-tile, work items of a replica, workgroups over all
        replicas): what the library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(steps[count, B] int64, sums[count, B, Q, c_z, c_y, c_x]) of the samples first ... first + count - 1 (count
        None: all from `first`); the variables first, then the pairs; synchronises the owner's stream."""
        first, count, b, steps = self._window(first, count)
        cx, cy, cz, nq = self.geometry()[:4]
        sums = np.empty((max(count, 0), b, nq, cz, cy, cx))
        check(self.lib.bflbm_coarse_read(self._h, first, count, _ptr(sums), steps.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return steps, sums

    def means(self, first=0, count=None):
        """sums / (b_x b_y b_z) [count, B, Q, c_z, c_y, c_x]: the block averages."""
        return self.read(first, count)[1] / float(self.block_sites)

    def block_variance(self, pair_slot, first=0, count=None):
        """[count, B, c_z, c_y, c_x]: the covariance of the pair's two variables within every block, the mean of the
        product minus the product of the means (analysis.coarse_block_variance); for a pair (a, a) the block variance."""
        from . import analysis
        p = int(pair_slot)
        if not 0 <= p < len(self.pairs):
            raise ValueError(f"coarse_trace: pair slot {pair_slot!r} outside the {len(self.pairs)} pairs")
        sums = self.read(first, count)[1]
        a, b = self.pairs[p]
        return analysis.coarse_block_variance(sums[:, :, a], sums[:, :, b], sums[:, :, len(self.variables) + p], self.block_sites)

    def write_plotfiles(self, root, replica=0):
        """One AMReX-format plotfile directory per sample of `replica`, named plotfile.concatenate(root, step): the coarse
        cells are the box, the components the block sums under sum_names, the step the replica's counter at the sample
        (two samples of one step share a directory: the later one stays).  plotfile.read_plotfile reads them back.
        Returns the directory names."""
        from . import plotfile
        steps, sums = self.read()
        if not 0 <= int(replica) < sums.shape[1]:
            raise ValueError(f"coarse_trace: replica {replica!r} outside the {sums.shape[1]} replicas")
        return [plotfile.write_plotfile(plotfile.concatenate(root, int(s[replica])), frame[replica], self.sum_names, time=float(s[replica]), step=int(s[replica]))
                for s, frame in zip(steps, sums)]


class LagTrace(_FieldRecorder):
    """Two-time correlations of chosen hydrovs / hydrovsbar variables against `origins` time origins kept on the device,
    for every replica, recorded every `every` steps through the owner (a lone single-slab BinaryLBM or a BatchLBM; no
    rings) and read once: include/bflbm.h, "Lag traces"; analysis.lag_record is the same rule in numpy.  Every
    `origin_stride`-th sample takes an origin (a copy of the variables of every site) into the next of the slots; every
    sample records, per held origin, corr = sum_x a(x, now) * b(x, origin) for every pair (a, b) and, with
    persist=(variable, level), the sites whose side of the level has not changed at any sample since the origin.  Made by
    owner.lag_trace(); an owner may carry several.  Closing the owner detaches the trace: it stays readable until its own
    close()."""
    _abi, _label = "bflbm_lag", "lag_trace"
    _geometry_types = (ctypes.c_int,) * 7 + (ctypes.c_longlong,) * 2

    def __init__(self, owner, create, variables, pairs, origins, origin_stride, persist, source, every, capacity):
        selection = self._select(source, variables, pairs)   # a lone name among the pairs: the variable with itself
        if persist is None:
            self.persist_slot, self.persist_level = -1, 0.0
        else:
            try:
                which, level = persist
            except (TypeError, ValueError):
                raise ValueError(f"lag_trace: persist = (variable, level) or None, got {persist!r}") from None
            self.persist_slot, self.persist_level = self._slot(which), float(level)
        self.origins, self.origin_stride = int(origins), int(origin_stride)
        super().__init__(owner, create, self.source, *selection, self.origins, self.origin_stride, self.persist_slot, self.persist_level,
                         int(every), int(capacity))
        self.sites = owner.n[0] * owner.n[1] * owner.n[2]

    names = property(_FieldRecorder._recorded_names, doc="The recorded variables by name, in slot order.")

    def geometry(self):
        """(nvars, npairs, origins R, origin_stride E, words W of a replica's sample, sites of a tile, tiles of a plane,
        bytes of the origins, bytes of the masks): what the library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(steps[count, B] int64, now[count, B, nvars], origin_steps[count, B, R] int64 (-1: an empty slot),
        alive[count, B, R] int64 (-1: no persistence, or an empty slot), corr[count, B, R, npairs] (NaN: an empty slot)) of
        the samples first ... first + count - 1 (count None: all from `first`): views of the sample's 8-byte words;
        synchronises the owner's stream."""
        first, count, b, steps = self._window(first, count)
        nv, npairs, r = len(self.variables), len(self.pairs), self.origins
        words = np.empty((max(count, 0), b, nv + r * (2 + npairs)))
        check(self.lib.bflbm_lag_read(self._h, first, count, _ptr(words), steps.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        slots = words[..., nv:].reshape(words.shape[0], b, r, 2 + npairs)
        return steps, words[..., :nv], slots[..., 0].view(np.int64), slots[..., 1].view(np.int64), slots[..., 2:]

    def _pair_index(self, pair):
        if isinstance(pair, (int, np.integer)):
            p = int(pair)
            if not 0 <= p < len(self.pairs):
                raise ValueError(f"lag_trace: pair {pair!r} outside the {len(self.pairs)} pairs")
            return p
        want = (self._slot(pair), self._slot(pair)) if isinstance(pair, str) else (self._slot(pair[0]), self._slot(pair[1]))
        if want not in self.pairs:
            raise ValueError(f"lag_trace: {pair!r} is not one of the recorded pairs")
        return self.pairs.index(want)

    def correlation(self, pair, connected=False, replica=0):
        """(lags in steps, the mean of corr over the origins at every lag, the origins per lag) of one pair (by index,
        by (a, b) of names or slots, or a lone name) and one replica; connected: minus now_a(sample) now_b(origin's
        sample) / sites (analysis.lag_connected), where the origin's own sample is in the record."""
        from . import analysis
        p = self._pair_index(pair)
        steps, now, osteps, _, corr = self.read()
        k = int(replica)
        values = corr[:, k, :, p]
        if connected:
            a, b = self.pairs[p]
            values = analysis.lag_connected(steps[:, k], osteps[:, k], values, now[:, k, a], now[:, k, b], self.sites)
        return analysis.lag_average(steps[:, k], osteps[:, k], values)

    def persistence(self, replica=0):
        """(lags in steps, the mean over the origins of alive / sites at every lag, the origins per lag) of one replica."""
        from . import analysis
        if self.persist_slot < 0:
            raise ValueError("lag_trace: made without persist=(variable, level)")
        steps, _, osteps, alive, _ = self.read()
        k = int(replica)
        values = np.where(alive[:, k] >= 0, alive[:, k] / float(self.sites), np.nan)
        return analysis.lag_average(steps[:, k], osteps[:, k], values)


MOMENT_MODES, MOMENT_WORDS = 19, 95


class MomentTrace(_Recorder):
    """The box sums of all 19 kinetic moments m = M f of both fluids, of their squares and of the products of the two
    fluids' moments mode by mode, for every replica, recorded on the device every `every` steps through the owner (a lone
    single-slab BinaryLBM or a BatchLBM; no rings) and read once: include/bflbm.h, "Moment traces";
    analysis.moment_record is the same arithmetic in numpy, analysis.moment_variances, analysis.equipartition and
    analysis.stress_series turn a record into the variance per mode, the equipartition ratios and the Green-Kubo input.
    Made by owner.moment_trace(); an owner may carry several.  Closing the owner detaches the trace: it stays readable
    until its own close()."""
    _abi = "bflbm_moment"
    _geometry_types = (ctypes.c_int,) * 3

    def __init__(self, owner, create, every, capacity):
        super().__init__(owner, create, int(every), int(capacity))
        self.sites = owner.n[0] * owner.n[1] * owner.n[2]

    def _owner_closing(self):
        """The owner's close(): the library detaches the trace; what it recorded stays readable until close()."""
        _unregister(self.owner, self)

    def geometry(self):
        """(words W of a replica's sample, sites of a tile, tiles of a plane): what the library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(steps[count, B] int64, sums[count, B, 95]) of the samples first ... first + count - 1 (count None: all from
        `first`); synchronises the owner's stream."""
        first, count, b, steps = self._window(first, count)
        sums = np.empty((max(count, 0), b, MOMENT_WORDS))
        check(self.lib.bflbm_moment_read(self._h, first, count, _ptr(sums), steps.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return steps, sums

    @staticmethod
    def _fluid(fluid):
        k = {"f": 0, "g": 1}.get(fluid, fluid)
        if k not in (0, 1):
            raise ValueError(f"moment_trace: fluid {fluid!r}, expected 0 / 'f' or 1 / 'g'")
        return int(k)

    def sums(self, fluid, first=0, count=None):
        """sum_x m_a(x) of one fluid (0 / "f" or 1 / "g"): [count, B, 19]."""
        k = self._fluid(fluid)
        return self.read(first, count)[1][..., MOMENT_MODES * k:MOMENT_MODES * (k + 1)]

    def squares(self, fluid, first=0, count=None):
        """sum_x m_a(x)^2 of one fluid: [count, B, 19]."""
        k = self._fluid(fluid)
        return self.read(first, count)[1][..., MOMENT_MODES * (2 + k):MOMENT_MODES * (3 + k)]

    def cross(self, first=0, count=None):
        """sum_x mf_a(x) mg_a(x): [count, B, 19]."""
        return self.read(first, count)[1][..., 4 * MOMENT_MODES:]


class ClusterTrace(_FieldRecorder):
    """The connected components of the set {v >= level} (side "above") or {v < level} (side "below") of one hydrovs /
    hydrovsbar variable at 1 to 8 levels under 6- or 26-connectivity on the periodic box, for every replica, labelled on
    the device by a union-find and recorded as 38 64-bit integers per level every `every` steps through the owner (a lone
    single-slab BinaryLBM or a BatchLBM; no rings) and read once: include/bflbm.h, "Cluster traces";
    analysis.cluster_record and analysis.cluster_labels are the same rule in numpy.  Made by owner.cluster_trace(); an
    owner may carry several.  Closing the owner detaches the trace: it stays readable until its own close()."""
    _abi, _label = "bflbm_cluster", "cluster_trace"
    _geometry_types = (ctypes.c_int,) * 7
    _alias = FieldStats._alias

    def __init__(self, owner, create, variable, levels, side, connectivity, source, every, capacity):
        if side not in MORPH_SIDES and side not in MORPH_SIDES.values():
            raise ValueError(f"cluster_trace: side {side!r}, expected 'above' (0) or 'below' (1)")
        if connectivity not in (6, 26):
            raise ValueError(f"cluster_trace: connectivity must be 6 or 26 (got {connectivity!r})")
        if not isinstance(variable, (str, int, np.integer)):
            raise ValueError(f"cluster_trace: one variable by name or component index, got {variable!r}")
        self._select(source, variable)
        self.side, self.connectivity = int(MORPH_SIDES.get(side, side)), int(connectivity)
        self.levels = np.atleast_1d(np.asarray(levels, dtype=np.float64)).copy()
        if self.levels.ndim != 1:
            raise ValueError(f"cluster_trace: levels is a number or a list of 1..8 numbers, got shape {self.levels.shape}")
        lv = self.levels if len(self.levels) else np.zeros(1)
        super().__init__(owner, create, self.source, self.variables[0], len(self.levels), _ptr(lv), self.side, self.connectivity,
                         int(every), int(capacity))
        self.n = tuple(owner.n)

    names = property(_FieldRecorder._recorded_names, doc="The recorded variable by name, a list of one.")

    def geometry(self):
        """(levels, connectivity, the brick's extents along x, y, z, bricks per replica, launches per level): what the
        library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(steps[count, B] int64, record[count, B, nlevels, 38] int64: ncomp, V, smax, the largest component's label,
        the sum of s^2, capped and the 32 bins of sizes in powers of two) of the samples first ... first + count - 1
        (count None: all from `first`); synchronises the owner's stream.  Raises BflbmError where a device loop hit its
        iteration cap (word 5 is not zero): such a record is not to be trusted."""
        first, count, b, steps = self._window(first, count)
        record = np.empty((max(count, 0), b, len(self.levels), 38), dtype=np.int64)
        as_ll = ctypes.POINTER(ctypes.c_longlong)
        check(self.lib.bflbm_cluster_read(self._h, first, count, record.ctypes.data_as(as_ll), steps.ctypes.data_as(as_ll)))
        if record[..., 5].any():
            raise _lib.BflbmError(f"cluster_trace: {int(record[..., 5].sum())} device loops hit their iteration cap")
        return steps, record

    def components(self, first=0, count=None):
        """[count, B, nlevels] int64: the number of components."""
        return self.read(first, count)[1][..., 0]

    def largest(self, first=0, count=None):
        """(smax[count, B, nlevels], label[count, B, nlevels]) int64: the size of the largest component and its label
        (0 and -1 where there is none)."""
        rec = self.read(first, count)[1]
        return rec[..., 2], rec[..., 3]

    def size_histogram(self, first=0, count=None):
        """[count, B, nlevels, 32] int64: the components with 2^b <= s < 2^(b+1)."""
        return self.read(first, count)[1][..., 6:]

    def mean_sizes(self, first=0, count=None):
        """(number average V / ncomp, weight average sum s^2 / V), each [count, B, nlevels]; NaN where there is no
        component."""
        rec = self.read(first, count)[1].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (np.where(rec[..., 0] > 0, rec[..., 1] / rec[..., 0], np.nan), np.where(rec[..., 1] > 0, rec[..., 4] / rec[..., 1], np.nan))

    def labels(self, level_index=0):
        """[B, nz, ny, nx] int32: the canonical labels of the owner's resident state now at one level (the smallest linear
        index of a site's component, -1 where unoccupied); records no sample; synchronises the owner's stream."""
        b = self._count()[1]
        out = np.empty((b, self.n[2], self.n[1], self.n[0]), dtype=np.int32)
        check(self.lib.bflbm_cluster_labels(self._h, int(level_index), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out


class ComponentTrace(_FieldRecorder):
    """Per connected component of the set {v >= level} (side "above") or {v < level} (side "below") of one hydrovs /
    hydrovsbar variable at 1 to 8 levels (the cluster trace's components and labels): size, a periodic-safe origin, the
    extent along every axis, the integer first and second moments about the origin and the area in cell faces of the
    `rows` components of at least `min_size` sites with the smallest labels, for every replica, recorded on the device
    as 64-bit integers every `every` steps through the owner (a lone single-slab BinaryLBM or a BatchLBM; no rings) and
    read once: include/bflbm.h, "Component traces"; analysis.component_table is the same rule in numpy.  Made by
    owner.component_trace(); an owner may carry several.  Closing the owner detaches the trace: it stays readable until
    its own close()."""
    _abi, _label = "bflbm_component", "component_trace"
    _geometry_types = (ctypes.c_int, ctypes.c_int, ctypes.c_longlong) + (ctypes.c_int,) * 4
    _alias = FieldStats._alias

    def __init__(self, owner, create, variable, levels, side, connectivity, min_size, rows, source, every, capacity):
        if side not in MORPH_SIDES and side not in MORPH_SIDES.values():
            raise ValueError(f"component_trace: side {side!r}, expected 'above' (0) or 'below' (1)")
        if connectivity not in (6, 26):
            raise ValueError(f"component_trace: connectivity must be 6 or 26 (got {connectivity!r})")
        if not isinstance(variable, (str, int, np.integer)):
            raise ValueError(f"component_trace: one variable by name or component index, got {variable!r}")
        self._select(source, variable)
        self.side, self.connectivity = int(MORPH_SIDES.get(side, side)), int(connectivity)
        self.min_size, self.rows = int(min_size), int(rows)
        self.levels = np.atleast_1d(np.asarray(levels, dtype=np.float64)).copy()
        if self.levels.ndim != 1:
            raise ValueError(f"component_trace: levels is a number or a list of 1..8 numbers, got shape {self.levels.shape}")
        lv = self.levels if len(self.levels) else np.zeros(1)
        super().__init__(owner, create, self.source, self.variables[0], len(self.levels), _ptr(lv), self.side, self.connectivity,
                         self.min_size, self.rows, int(every), int(capacity))
        self.n = tuple(owner.n)

    names = property(_FieldRecorder._recorded_names, doc="The recorded variable by name, a list of one.")

    def geometry(self):
        """(levels, connectivity, min_size, rows, header words, row words, launches per level): what the library built."""
        return self._geometry()

    def read(self, first=0, count=None):
        """(steps[count, B] int64, header[count, B, nlevels, 6] int64: ncomp, V, nqual, Vqual, nrows, capped,
        rows[count, B, nlevels, rows, 18] int64: label, size, origin, extent, sum d, sum d^2, sum dx dy, dx dz, dy dz,
        faces) of the samples first ... first + count - 1 (count None: all from `first`); synchronises the owner's
        stream.  Raises BflbmError where a device loop hit its iteration cap (header word 5 is not zero)."""
        first, count, b, steps = self._window(first, count)
        record = np.empty((max(count, 0), b, len(self.levels), 6 + self.rows * 18), dtype=np.int64)
        as_ll = ctypes.POINTER(ctypes.c_longlong)
        check(self.lib.bflbm_component_read(self._h, first, count, record.ctypes.data_as(as_ll), steps.ctypes.data_as(as_ll)))
        if record[..., 5].any():
            raise _lib.BflbmError(f"component_trace: {int(record[..., 5].sum())} device loops hit their iteration cap")
        return steps, record[..., :6].copy(), record[..., 6:].reshape(record.shape[:3] + (self.rows, 18)).copy()

    def _rows(self, first, count):
        return self.read(first, count)[2]

    def sizes(self, first=0, count=None):
        """[count, B, nlevels, rows] int64: the sizes, 0 in unused rows."""
        return self._rows(first, count)[..., 1]

    def labels_of_rows(self, first=0, count=None):
        """[count, B, nlevels, rows] int64: the canonical labels, -1 in unused rows."""
        return self._rows(first, count)[..., 0]

    def spans(self, first=0, count=None):
        """[count, B, nlevels, rows, 3] bool: the component covers every coordinate of the axis (x, y, z): necessary for
        wrapping around it, not sufficient.  False in unused rows."""
        t = self._rows(first, count)
        return (t[..., 0:1] >= 0) & (t[..., 5:8] == np.asarray(self.n))

    def areas(self, first=0, count=None):
        """[count, B, nlevels, rows] int64: the faces towards unoccupied sites."""
        return self._rows(first, count)[..., 17]

    def centroids(self, first=0, count=None):
        """[count, B, nlevels, rows, 3]: the centroids (x, y, z) in cell indices, like Trace.com();
        NaN along a spanned axis and in unused rows (analysis.component_centroids)."""
        from . import analysis
        return analysis.component_centroids(self._rows(first, count), self.n)

    def gyration(self, first=0, count=None):
        """[count, B, nlevels, rows, 3, 3] float64: the central second-moment tensors (analysis.component_gyration)."""
        from . import analysis
        return analysis.component_gyration(self._rows(first, count))


class RadialTrace(_FieldRecorder):
    """The sums of chosen hydrovs / hydrovsbar variables, of chosen products of them and of chosen projections onto the
    outward radial unit vector over the shells of width `delta` about a droplet's centre (a fixed one, or the centre of
    mass of the cells above a threshold), for every replica, recorded on the device every `every` steps through the owner
    (a lone single-slab BinaryLBM or a BatchLBM) and read once: include/bflbm.h, "Radial traces"; analysis.radial_shells
    is the same arithmetic in numpy, analysis.radial_pressure, pressure_jump, radial_force_integral, fit_radial_profile
    and equimolar_radius turn the shell means into the Laplace-law inputs.  Made by owner.radial_trace(); an owner may
    carry several.  Closing the owner detaches the trace: it stays readable until its own close()."""
    _abi, _label = "bflbm_radial", "radial_trace"

    def __init__(self, owner, create, variables, pairs, radials, centre, threshold, delta, nbins, source, every, capacity):
        selection = self._select(source, variables, pairs)   # a lone name among the pairs: its square
        self.radials = [(-1 if w is None else self._slot(w), tuple(self._slot(c) for c in v)) for w, v in radials]
        if any(len(v) != 3 for _, v in self.radials):
            raise ValueError("radial_trace: a radial term is (w, (vx, vy, vz)), w a variable or None")
        self.delta = float(delta)
        if not (np.isfinite(self.delta) and self.delta > 0):
            raise ValueError(f"radial_trace: delta {delta} must be finite and > 0")
        if nbins is None:                                  # the shells that cover half the box diagonal
            nbins = min(128, int(np.floor(0.5 * np.sqrt(float(sum(v * v for v in owner.n))) / self.delta)) + 1)
        rw, rv = _ints(w for w, _ in self.radials), _ints(c for _, v in self.radials for c in v)
        c = None if centre is None else (ctypes.c_double * 3)(*[float(v) for v in centre])
        thr = -np.inf if threshold is None else float(threshold)
        super().__init__(owner, create, self.source, *selection, len(self.radials), rw, rv, c, thr, self.delta, int(nbins),
                         int(every), int(capacity))

    names = property(_FieldRecorder._recorded_names, doc="The recorded variables by name, in slot order: what analysis.radial_pressure takes.")

    def geometry(self):
        """(Q = variables + pairs + radial terms, shells, sites of a tile, tiles per plane): what the library built."""
        return self._geometry()

    @property
    def r(self):
        """The shell radii (k + 1/2) delta, [nbins], in cells."""
        return (np.arange(self.geometry()[1]) + 0.5) * self.delta

    def read(self, first=0, count=None):
        """(centres[count, B, 3], counts[count, B, nbins], sums[count, B, Q, nbins], steps[count, B] int64) of the samples
        first ... first + count - 1 (count None: all from `first`): the centre used in cell indices, the sites of every
        shell, the sums of the variables, then the pairs, then the radial terms; synchronises the owner's stream."""
        first, count, b, steps = self._window(first, count)
        nq, nbins = self.geometry()[:2]
        rec = np.empty((max(count, 0), b, 3 + (1 + nq) * nbins))
        check(self.lib.bflbm_radial_read(self._h, first, count, _ptr(rec), steps.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return rec[..., :3], rec[..., 3:3 + nbins], rec[..., 3 + nbins:].reshape(rec.shape[:2] + (nq, nbins)), steps

    def means(self, first=0, count=None):
        """sums / counts [count, B, Q, nbins]: the shell averages, NaN where a shell holds no site."""
        _, counts, sums, _ = self.read(first, count)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(counts[..., None, :] > 0, sums / counts[..., None, :], np.nan)


# kernel schedules of include/bflbm.h (bflbm_set_schedule): "fused" = plane march with the ring densities pulled
# (bit-exact), "handover" = plane march with the ring densities handed over from the previous step (tolerance)
SCHEDULES = {"two_pass": 0, "fused": 1, "fused_exact": 1, "auto": 2, "handover": 3}


class BinaryLBM(_DropletMixin):
    _droplet_fn = ("bflbm_droplet_moments", "bflbm_fit_droplet", "bflbm_fit_droplet_flow")

    """One z-slab [z0, z1) of a periodic nx*ny*nz D3Q19 binary-fluid lattice on one GPU."""

    def __init__(self, nx, ny=None, nz=None, params=None, z0=0, z1=None, rank=0, nranks=1,
                 device=0, schedule=None, stream=None):
        self.lib = _lib.load()
        ny = nx if ny is None else ny
        nz = nx if nz is None else nz
        z1 = nz if z1 is None else z1
        self.n = (int(nx), int(ny), int(nz))
        self.z0, self.z1 = int(z0), int(z1)
        self.nzl = self.z1 - self.z0
        self.rank, self.nranks = int(rank), int(nranks)
        self.params = params if params is not None else default_params()
        dom = Domain()
        dom.n[0], dom.n[1], dom.n[2] = self.n
        dom.z0, dom.z1, dom.rank, dom.nranks, dom.device = self.z0, self.z1, self.rank, self.nranks, int(device)
        h = ctypes.c_void_p()
        check(self.lib.bflbm_create(ctypes.byref(self.params), ctypes.byref(dom), ctypes.byref(h)))
        self._h = h
        if stream is not None:      # an external hipStream_t handle; 0 is the legacy default stream
            check(self.lib.bflbm_set_stream(self._h, ctypes.c_void_p(stream), 1))
        if schedule is not None:
            self.set_schedule(schedule)

    @classmethod
    def _borrow(cls, handle, n, z0, z1, rank, nranks, params):
        """View on a context owned by someone else (a slab of a RingLBM); close() does not destroy it."""
        self = cls.__new__(cls)
        self.lib = _lib.load()
        self.n, self.z0, self.z1, self.nzl = tuple(n), int(z0), int(z1), int(z1) - int(z0)
        self.rank, self.nranks, self.params = int(rank), int(nranks), params
        self._h, self._borrowed = handle, True
        return self

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            for d in list(getattr(self, "_dependents", [])):   # e.g. structure-factor accumulators living on this context:
                getattr(d, "_owner_closing", d.close)()        # closed; a spectrum trace: detached by the library, still readable
            if not getattr(self, "_borrowed", False):
                self.lib.bflbm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- configuration (the reference edits source-level globals) ---------------------------
    def set_params(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise AttributeError(f"unknown model parameter {k!r}")
            setattr(self.params, k, v)
        check(self.lib.bflbm_set_params(self._h, ctypes.byref(self.params)))

    def set_schedule(self, schedule):
        code = SCHEDULES.get(schedule, schedule)
        check(self.lib.bflbm_set_schedule(self._h, int(code)))

    # -- shapes ----------------------------------------------------------------------------
    def resolved_schedule(self):
        """Name of the schedule the next step runs (auto resolved for the current parameters and lattice)."""
        v = ctypes.c_int()
        check(self.lib.bflbm_resolved_schedule(self._h, ctypes.byref(v)))
        return {0: "two_pass", 1: "fused", 3: "handover"}[v.value]

    @property
    def slab_shape(self):
        return (self.nzl, self.n[1], self.n[0])

    def slab_fab(self):
        """FAB descriptor of a ghost-free array covering exactly this slab."""
        lo = (0, 0, self.z0)
        hi = (self.n[0] - 1, self.n[1] - 1, self.z1 - 1)
        return make_fab(lo, hi)

    def _new(self, ncomp):
        return np.empty((ncomp,) + self.slab_shape, dtype=np.float64)

    # -- initial conditions ------------------------------------------------------------------
    def LBM_init_mixture(self):
        check(self.lib.bflbm_init_mixture(self._h))

    def LBM_init_stripe(self, frac):
        check(self.lib.bflbm_init_stripe(self._h, float(frac)))

    def LBM_init_droplet(self, r):
        check(self.lib.bflbm_init_droplet(self._h, float(r)))

    def upload(self, f0, g0, fab=None):
        """Stage populations of one box (mf.ParallelCopy(mf0), LBM_binary.H:643)."""
        if fab is None:
            _check_array(f0, NVEL, self.slab_shape, "f0")
            _check_array(g0, NVEL, self.slab_shape, "g0")
            fab = self.slab_fab()
        check(self.lib.bflbm_upload_fg(self._h, _ptr(f0), _ptr(g0), ctypes.byref(fab)))

    def commit_upload(self, reset_step_counter=True):
        check(self.lib.bflbm_commit_upload(self._h, int(bool(reset_step_counter))))

    def LBM_init(self, f0, g0, fab=None):
        """Continue from given populations (LBM_binary.H:632-661); single slab only --
        multi-slab callers use SlabLattice.LBM_init which exchanges the z faces."""
        if self.nranks != 1:
            raise _lib.BflbmError("BinaryLBM.LBM_init needs the slab driver when nranks > 1")
        self.upload(f0, g0, fab)
        self.commit_upload(True)

    # -- time stepping ---------------------------------------------------------------------
    def LBM_timestep(self, nsteps=1):
        check(self.lib.bflbm_step(self._h, int(nsteps)))

    def step_boundary(self):
        check(self.lib.bflbm_step_boundary(self._h))

    def step_interior(self):
        check(self.lib.bflbm_step_interior(self._h))

    def step_finish(self):
        check(self.lib.bflbm_step_finish(self._h))

    @property
    def steps_done(self):
        n = ctypes.c_longlong()
        check(self.lib.bflbm_step_count(self._h, ctypes.byref(n)))
        return n.value

    def set_steps_done(self, n):
        """Absolute step of the resident state = noise index of the next step (restart from a kBT > 0 checkpoint)."""
        check(self.lib.bflbm_set_step_count(self._h, int(n)))

    def placement_report(self):
        """What the placement tuning at creation measured (bflbm_tune_placement): ms per step of every candidate allocation
        tried and the index of the one kept; None when the context was never tuned (small lattices, BFLBM_PLACEMENT_CANDIDATES=1)."""
        ms = (ctypes.c_float * 8)()
        n, k = ctypes.c_int(), ctypes.c_int()
        check(self.lib.bflbm_placement_report(self._h, ms, ctypes.byref(n), ctypes.byref(k)))
        return None if n.value == 0 else {"candidates_ms_per_step": [round(float(v), 4) for v in list(ms)[:n.value]], "kept": k.value}

    def tune_placement(self, max_candidates=3):
        """Draw the physical placement of the state again (leaves the context as freshly created: call before an init)."""
        check(self.lib.bflbm_tune_placement(self._h, int(max_candidates), None, None))
        return self.placement_report()

    @property
    def state_total_max(self):
        """Largest |rho + phi| of the state the last LBM_init(f0, g0) made resident (what `auto` keys its stability bound
        on); negative after an analytic init, where rho_hi + rho_lo of the parameters is that number."""
        v = ctypes.c_double()
        check(self.lib.bflbm_state_total_max(self._h, ctypes.byref(v)))
        return v.value

    def set_state_total_max(self, v):
        check(self.lib.bflbm_set_state_total_max(self._h, float(v)))

    # -- state and per-step fields -------------------------------------------------------------
    def populations(self, f=None, g=None, fab=None):
        """fold, gold valid cells (post-stream state of the last completed step)."""
        if fab is None:
            f = self._new(NVEL) if f is None else f
            g = self._new(NVEL) if g is None else g
            fab = self.slab_fab()
        check(self.lib.bflbm_download_fg(self._h, _ptr(f), _ptr(g), ctypes.byref(fab)))
        return f, g

    def LBM_hydrovars_density(self, out=None, fab=None, ncomp=NHYDROBAR):
        if fab is None:
            out = self._new(ncomp) if out is None else out
            fab = self.slab_fab()
        check(self.lib.bflbm_get_hydrovsbar(self._h, _ptr(out), int(ncomp), ctypes.byref(fab)))
        return out

    def LBM_hydrovars(self, out=None, fab=None, ncomp=NHYDRO):
        if fab is None:
            out = self._new(ncomp) if out is None else out
            fab = self.slab_fab()
        check(self.lib.bflbm_get_hydrovs(self._h, _ptr(out), int(ncomp), ctypes.byref(fab)))
        return out

    def thermal_noise(self, fn=None, gn=None, fab=None):
        if fab is None:
            fn = self._new(NVEL) if fn is None else fn
            gn = self._new(NVEL) if gn is None else gn
            fab = self.slab_fab()
        check(self.lib.bflbm_get_noise(self._h, _ptr(fn), _ptr(gn), ctypes.byref(fab)))
        return fn, gn

    def inject_noise(self, fn, gn, fab=None):
        """Test hook: the next step's collision uses these noise moments."""
        if fn is None:
            check(self.lib.bflbm_inject_noise(self._h, None, None, None))
            return
        if fab is None:
            _check_array(fn, NVEL, self.slab_shape, "fn")
            _check_array(gn, NVEL, self.slab_shape, "gn")
            fab = self.slab_fab()
        check(self.lib.bflbm_inject_noise(self._h, _ptr(fn), _ptr(gn), ctypes.byref(fab)))

    # -- reductions -------------------------------------------------------------------------
    def trace(self, every, capacity, threshold=None):
        """Record the droplet moments of the cells with rho > threshold (None: every cell) after every `every`-th step."""
        return Trace(self, "bflbm_trace_create", every, capacity, threshold)

    def interface_trace(self, level, field="rho", window=None, every=1, capacity=64):
        """Record, after every `every`-th step, the rising and falling height of the `field` = level contour ("rho" or
        "phi") above every column, scanned over the planes window = (z_lo, z_hi) (None: all): InterfaceTrace.
        The device buffer of `capacity` samples is allocated at once: capacity x 2 ny nx doubles (the default 64 takes
        256 MiB on a 512 x 512 column lattice); a step whose sample would not fit is refused, so size it for the run."""
        return InterfaceTrace(self, "bflbm_iface_create", level, field, window, every, capacity)

    def shape_trace(self, level, nodes=None, field="rho", direction="falling", centre=None, threshold=None, step=0.5, rmax=None, every=1, capacity=64):
        """Record, after every `every`-th step, the radius at which the `field` ("rho" or "phi") falls (or, direction
        "rising", rises) through `level` along fixed rays from a centre: ShapeTrace.  nodes = (dirs[ndir, 3], weights[ndir])
        (None: analysis.ray_nodes(16, 32)); centre: a fixed one in cell indices (x, y, z), or None for the centre of mass of
        the cells with rho > threshold (None: every cell), which is Trace.com() of the same state; the rays are sampled
        every `step` cells out to rmax (None: half the smallest extent)."""
        return ShapeTrace(self, "bflbm_shape_create", level, nodes, field, direction, centre, threshold, step, rmax, every, capacity)

    def spectrum_trace(self, var_names_or_pairs, kind="shell", every=1, capacity=64, lb_hydrovars=False, zero_avg=True, var_scaling=None):
        """Record, after every `every`-th step, the structure factor of pairs of hydrovs (lb_hydrovars: hydrovsbar)
        variables binned into shells in |q| (kind "shell") or into |k| along one axis ("x", "y", "z"): SpectrumTrace.
        Variable names form the pairs of structfact.StructFact; a list of index pairs (a, b) is taken as it is."""
        return SpectrumTrace(self, "bflbm_spectrum_create", var_names_or_pairs, kind, every, capacity, lb_hydrovars, zero_avg, var_scaling)

    def mode_trace(self, variables, modes, every=1, capacity=64, lb_hydrovars=False):
        """Record, after every `every`-th step, the Fourier amplitudes of hydrovs (lb_hydrovars: hydrovsbar) variables,
        given by name (plotfile.variable_names) or index, at the integer wavevectors modes[nmodes, 3] = (mx, my, mz):
        ModeTrace.  `capacity` samples of nvars x nmodes complex numbers are allocated at creation."""
        return ModeTrace(self, "bflbm_modes_create", variables, modes, every, capacity, lb_hydrovars)

    def field_stats(self, variables, pairs=(), source="hydrovs", every=0):
        """Accumulate, at every site, the mean over frames of up to 8 variables of `source` ("hydrovs", "hydrovsbar" or
        "noise"; names or component indices) and the covariance of up to 16 pairs of them (names or slots; a lone name is
        its variance): FieldStats.  A frame is taken after every `every`-th step; every = 0: by sample() only."""
        return FieldStats(self, "bflbm_fstat_create", variables, pairs, source, every)

    def profile_trace(self, variables, pairs=(), axis="z", source="hydrovs", every=1, capacity=64):
        """Record, after every `every`-th step, the sums over every lattice plane normal to `axis` ("x", "y", "z") of up
        to 8 variables of `source` ("hydrovs" or "hydrovsbar"; names or component indices) and of the products of up to
        16 pairs of them (names or slots; a lone name is its square): ProfileTrace."""
        return ProfileTrace(self, "bflbm_profile_create", variables, pairs, axis, source, every, capacity)

    def histogram_trace(self, ranges, pairs=(), source="hydrovs", every=1, capacity=64):
        """Counts of the sites of chosen variables over fixed bins and of pairs of them over two binnings, recorded on the
        device every `every` steps: ranges = {variable: (lo, hi, nbins)} of up to 8 variables of `source` ("hydrovs",
        "hydrovsbar" or "noise"), up to 4 pairs (a, b) of them by name or slot: HistogramTrace."""
        return HistogramTrace(self, "bflbm_hist_create", ranges, pairs, source, every, capacity)

    def morphology_trace(self, variable, levels, side="above", source="hydrovs", every=1, capacity=64):
        """Record, after every `every`-th step, the cubes, faces, edges and vertices of the set {variable >= level}
        (side "above") or {variable < level} (side "below") at 1 to 8 levels, one variable of `source` ("hydrovs" or
        "hydrovsbar") by name or component index: MorphologyTrace, whose functionals() are the volume, the interface
        area, twice the mean breadth and the Euler characteristic."""
        return MorphologyTrace(self, "bflbm_morph_create", variable, levels, side, source, every, capacity)

    def chord_trace(self, variable, levels, side="above", max_length=64, source="hydrovs", every=1, capacity=64):
        """Record, after every `every`-th step, the chord-length distributions along x, y and z of the set
        {variable >= level} (side "above") or {variable < level} (side "below") at 1 to 8 levels, one variable of
        `source` ("hydrovs" or "hydrovsbar") by name or component index; chords of max_length sites and more share the
        last bin: ChordTrace, whose hist(axis), chords(axis), spanning(axis) and mean_length(axis) cut the record up."""
        return ChordTrace(self, "bflbm_chord_create", variable, levels, side, max_length, source, every, capacity)

    def coarse_trace(self, variables, pairs=(), block=(1, 1, 1), origin=(0, 0, 0), extent=None, source="hydrovs", every=1, capacity=64):
        """Record, after every `every`-th step, the sums of the `variables` of `source` ("hydrovs" or "hydrovsbar"; names or
        component indices) and of the products of the `pairs` of them over the blocks of `block` = (b_x, b_y, b_z) sites of
        the periodic window that starts at `origin` and has `extent` sites (x, y, z; None: to the end of the box), as a
        time series of coarse fields on the device: CoarseTrace, whose read(), means(), block_variance(pair) and
        write_plotfiles(root) give the record.  Block (1, 1, 1) records the window itself: a slice or a sub-volume."""
        return CoarseTrace(self, "bflbm_coarse_create", variables, pairs, block, origin, extent, source, every, capacity)

    def lag_trace(self, variables, pairs, origins=8, origin_stride=1, persist=None, source="hydrovs", every=1, capacity=64):
        """Record, after every `every`-th step, the two-time correlations of the `variables` of `source` ("hydrovs" or
        "hydrovsbar"; names or component indices) against `origins` time origins kept on the device: every
        `origin_stride`-th sample takes an origin, every sample records sum_x a(x, now) * b(x, origin) per held origin and
        pair (a, b) of `pairs` (a lone name: the variable with itself) and, with persist=(variable, level), the sites whose
        side of the level has not changed since the origin: LagTrace, whose read(), correlation(pair) and persistence()
        give the record."""
        return LagTrace(self, "bflbm_lag_create", variables, pairs, origins, origin_stride, persist, source, every, capacity)

    def moment_trace(self, every=1, capacity=64):
        """Record, after every `every`-th step, the box sums of all 19 kinetic moments of both fluids, of their squares
        and of the products mf_a mg_a of the two fluids' moments, 95 doubles a sample, with one summing launch that reads
        the populations once and one finishing launch: MomentTrace, whose read(), sums(fluid), squares(fluid) and cross()
        give the record."""
        return MomentTrace(self, "bflbm_moment_create", every, capacity)

    def cluster_trace(self, variable, levels, side="above", connectivity=26, source="hydrovs", every=1, capacity=64):
        """Record, after every `every`-th step, the connected components of the set {variable >= level} (side "above") or
        {variable < level} (side "below") at 1 to 8 levels under 6- or 26-connectivity, one variable of `source`
        ("hydrovs" or "hydrovsbar") by name or component index: ClusterTrace, whose record holds the number of components,
        the largest, the sum of the squared sizes and a histogram of the sizes, and whose labels() are the components."""
        return ClusterTrace(self, "bflbm_cluster_create", variable, levels, side, connectivity, source, every, capacity)

    def component_trace(self, variable, levels, side="above", connectivity=26, min_size=1, rows=64, source="hydrovs", every=1, capacity=64):
        """Record, after every `every`-th step, per connected component of the set {v >= level} (or {v < level}) of one variable
        of `source` its place and shape (the components are cluster_trace's): ComponentTrace, whose record tabulates, per level, the `rows` components of at least `min_size` sites with
        the smallest labels: size, origin, extent, integer moments and area of each."""
        return ComponentTrace(self, "bflbm_component_create", variable, levels, side, connectivity, min_size, rows, source, every, capacity)

    def radial_trace(self, variables, pairs=(), radials=(), centre=None, threshold=None, delta=1.0, nbins=None, source="hydrovs",
                     every=1, capacity=64):
        """Record, after every `every`-th step, the sums over the shells of width `delta` (cells) about `centre` (cell
        indices; None: the centre of mass of the cells with rho above `threshold`, None: every cell) of up to 8 variables
        of `source` (names or component indices), of the products of up to 16 pairs of them and of up to 4 radial terms
        (w, (vx, vy, vz)) = w (v . r^), w None for the bare projection (names or slots), with the sites of every shell:
        RadialTrace.  nbins None: the shells that cover half the box diagonal, 128 at the most."""
        return RadialTrace(self, "bflbm_radial_create", variables, pairs, radials, centre, threshold, delta, nbins, source, every, capacity)

    def com_sums(self):
        s = (ctypes.c_double * 4)()
        check(self.lib.bflbm_com_sums(self._h, s))
        return np.array(list(s))

    def update_com(self):
        """Centre of mass of rho (LBM_hydrovs.H:26-60), single slab."""
        s = self.com_sums()
        return s[1:] / s[0]

    def mass(self):
        r, p = ctypes.c_double(), ctypes.c_double()
        check(self.lib.bflbm_mass(self._h, ctypes.byref(r), ctypes.byref(p)))
        return r.value, p.value

    # -- reference-state noise: the reference's USE_REF_STATE build (LBM_binary.H:12, :92-107) ---------
    def set_ref_state(self, rho_eq, phi_eq, rhot_eq, com_ref, fab=None):
        """Equilibrium fields over the GLOBAL lattice (nz, ny, nx) (main_run_job.cpp:216-235) and the
        reference centre of mass com_ref[0]; noise amplitudes then come from them."""
        n = self.n
        fab = fab if fab is not None else make_fab((0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1))
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (rho_eq, phi_eq, rhot_eq)]
        check(self.lib.bflbm_set_ref_state(self._h, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), ctypes.byref(fab)))
        c = (ctypes.c_double * 3)(*[float(v) for v in com_ref])
        check(self.lib.bflbm_enable_ref_state(self._h, 1, c))

    def disable_ref_state(self):
        check(self.lib.bflbm_enable_ref_state(self._h, 0, None))

    @property
    def ref_state_active(self):
        a = ctypes.c_int()
        check(self.lib.bflbm_ref_state_active(self._h, ctypes.byref(a)))
        return bool(a.value)

    def set_com(self, com):
        """Global centre of mass of the resident state, for a slab of a decomposed lattice."""
        c = (ctypes.c_double * 3)(*[float(v) for v in com])
        check(self.lib.bflbm_set_com(self._h, c))

    # -- halo exchange plumbing (used by slab.SlabLattice) ---------------------------------------
    def halo_bytes(self, kind=_lib.HALO_STATE):
        n = ctypes.c_size_t()
        check(self.lib.bflbm_halo_bytes(self._h, int(kind), ctypes.byref(n)))
        return n.value

    def halo_pack(self, kind, side, device_ptr):
        check(self.lib.bflbm_halo_pack(self._h, int(kind), int(side), ctypes.c_void_p(device_ptr)))

    def halo_unpack(self, kind, side, device_ptr):
        check(self.lib.bflbm_halo_unpack(self._h, int(kind), int(side), ctypes.c_void_p(device_ptr)))

    def halo_planes(self, kind, side, pack):
        """(device addresses of the 38 component planes of a face, bytes per plane): the staging-free exchange."""
        ptrs = (ctypes.c_void_p * 64)()
        nb, cnt = ctypes.c_size_t(), ctypes.c_int()
        check(self.lib.bflbm_halo_planes(self._h, int(kind), int(side), int(bool(pack)), ptrs, ctypes.byref(nb), ctypes.byref(cnt)))
        return [int(ptrs[k]) for k in range(cnt.value)], nb.value

    def halo_plane_tensors(self, kind, side, pack, device):
        """The same as torch tensors that alias the state buffer (zero-copy, through __cuda_array_interface__)."""
        import torch
        cache = self.__dict__.setdefault("_plane_views", {})
        ptrs, nb = self.halo_planes(kind, side, pack)
        out = []
        for p in ptrs:
            t = cache.get(p)
            if t is None:
                t = cache[p] = torch.as_tensor(_DevicePlane(p, nb // 8), device=device)
            out.append(t)
        return out

    # -- misc ------------------------------------------------------------------------------
    def sync(self):
        check(self.lib.bflbm_sync(self._h))

    def timer_start(self):
        check(self.lib.bflbm_timer_start(self._h))

    def timer_stop(self):
        ms = ctypes.c_float()
        check(self.lib.bflbm_timer_stop(self._h, ctypes.byref(ms)))
        return ms.value

    def debug_time_kernel(self, which, reps=10):
        """ms per launch of a calibration kernel (0 pull-copy, 1 density pass, 2 D2D memcpy)."""
        ms = ctypes.c_float()
        check(self.lib.bflbm_debug_time_kernel(self._h, int(which), int(reps), ctypes.byref(ms)))
        return ms.value

    def device_bytes(self):
        n = ctypes.c_size_t()
        check(self.lib.bflbm_device_bytes(self._h, ctypes.byref(n)))
        return n.value


class RingLBM(_DropletMixin):
    _droplet_fn = ("bflbm_ring_droplet_moments", "bflbm_ring_fit_droplet", "bflbm_ring_fit_droplet_flow")

    """The whole lattice as a ring of z-slabs driven by this one process through the native ring of the
    C-ABI (bflbm_ring_*): slab r on GPU devices[r % len(devices)], halo exchange by peer copies overlapped
    with the interior planes.  Same operator surface as BinaryLBM; fields are full-lattice arrays."""

    def __init__(self, nx, ny=None, nz=None, nslabs=1, devices=(0,), params=None, schedule=None):
        self.lib = _lib.load()
        ny = nx if ny is None else ny
        nz = nx if nz is None else nz
        self.n = (int(nx), int(ny), int(nz))
        self.params = params if params is not None else default_params()
        n3 = (ctypes.c_int * 3)(*self.n)
        dev = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        h = ctypes.c_void_p()
        check(self.lib.bflbm_ring_create(ctypes.byref(self.params), n3, int(nslabs), dev, len(devices), ctypes.byref(h)))
        self._h = h
        self.slabs = []
        for r in range(int(nslabs)):
            c = ctypes.c_void_p()
            check(self.lib.bflbm_ring_slab(self._h, r, ctypes.byref(c)))
            z0, z1 = (self.n[2] * r) // nslabs, (self.n[2] * (r + 1)) // nslabs
            self.slabs.append(BinaryLBM._borrow(c, self.n, z0, z1, r, nslabs, self.params))
        if schedule is not None:
            code = SCHEDULES.get(schedule, schedule)
            check(self.lib.bflbm_ring_set_schedule(self._h, int(code)))

    def close(self):
        if getattr(self, "_h", None):
            for d in list(getattr(self, "_dependents", [])):      # ring-level accumulators and the moments trace: closed;
                getattr(d, "_owner_closing", d.close)()           # a spectrum trace: detached by the library, still readable
            for s in self.slabs:
                for d in list(getattr(s, "_dependents", [])):
                    d.close()
            self.lib.bflbm_ring_destroy(self._h)
            self._h = None
            for s in self.slabs:
                s._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise AttributeError(f"unknown model parameter {k!r}")
            setattr(self.params, k, v)
        check(self.lib.bflbm_ring_set_params(self._h, ctypes.byref(self.params)))

    def set_schedule(self, schedule):
        """Every slab's schedule (BinaryLBM.set_schedule); slabs[0].resolved_schedule() says what the next step runs."""
        check(self.lib.bflbm_ring_set_schedule(self._h, int(SCHEDULES.get(schedule, schedule))))

    def LBM_init_mixture(self):
        check(self.lib.bflbm_ring_init_mixture(self._h))

    def LBM_init_stripe(self, frac):
        check(self.lib.bflbm_ring_init_stripe(self._h, float(frac)))

    def LBM_init_droplet(self, r):
        check(self.lib.bflbm_ring_init_droplet(self._h, float(r)))

    def LBM_init(self, f0, g0):
        """f0, g0: full-lattice arrays (19, nz, ny, nx); every slab takes its planes."""
        _check_array(f0, NVEL, (self.n[2], self.n[1], self.n[0]), "f0")
        _check_array(g0, NVEL, (self.n[2], self.n[1], self.n[0]), "g0")
        fab = make_fab((0, 0, 0), (self.n[0] - 1, self.n[1] - 1, self.n[2] - 1))
        for s in self.slabs:
            s.upload(f0, g0, fab)
        check(self.lib.bflbm_ring_commit_upload(self._h, 1))

    def LBM_timestep(self, nsteps=1):
        check(self.lib.bflbm_ring_step(self._h, int(nsteps)))

    # -- recorders: served by LBM_timestep, not by stepping the slabs by hand -----------------
    def trace(self, every, capacity, threshold=None):
        """Record the droplet moments of the cells with rho > threshold (None: every cell) after every `every`-th step:
        Trace, one replica, the record a lone lattice's bit for bit.  At most one per ring."""
        return Trace(self, "bflbm_ring_trace_create", every, capacity, threshold)

    def spectrum_trace(self, var_names_or_pairs, kind="shell", every=1, capacity=64, lb_hydrovars=False, zero_avg=True, var_scaling=None):
        """Record, after every `every`-th step, the binned structure factor of pairs of hydrovs (lb_hydrovars: hydrovsbar)
        variables by a slab FFT over the ring: SpectrumTrace, with the arguments of BinaryLBM.spectrum_trace."""
        return SpectrumTrace(self, "bflbm_ring_spectrum_create", var_names_or_pairs, kind, every, capacity, lb_hydrovars, zero_avg, var_scaling)

    def field_stats(self, variables, pairs=(), source="hydrovs", every=0):
        """Per-site means and covariances over frames (BinaryLBM.field_stats); every slab keeps the accumulators of its
        own planes on its own device, the values are a lone lattice's bit for bit."""
        return FieldStats(self, "bflbm_ring_fstat_create", variables, pairs, source, every)

    def profile_trace(self, variables, pairs=(), axis="z", source="hydrovs", every=1, capacity=64):
        """Plane sums of variables and products along one axis (BinaryLBM.profile_trace): every slab sums its own planes,
        slab 0 finishes; the record is a lone lattice's bit for bit."""
        return ProfileTrace(self, "bflbm_ring_profile_create", variables, pairs, axis, source, every, capacity)

    def histogram_trace(self, ranges, pairs=(), source="hydrovs", every=1, capacity=64):
        """Bin counts of variables and pairs (BinaryLBM.histogram_trace): every slab counts its own planes, slab 0 adds
        the slabs' totals."""
        return HistogramTrace(self, "bflbm_ring_hist_create", ranges, pairs, source, every, capacity)

    def _gather(self, ncomp, call):
        out = np.empty((ncomp, self.n[2], self.n[1], self.n[0]))
        fab = make_fab((0, 0, 0), (self.n[0] - 1, self.n[1] - 1, self.n[2] - 1))
        for s in self.slabs:
            call(s, out, fab)
        return out

    def populations(self):
        f = np.empty((NVEL, self.n[2], self.n[1], self.n[0])); g = np.empty_like(f)
        fab = make_fab((0, 0, 0), (self.n[0] - 1, self.n[1] - 1, self.n[2] - 1))
        for s in self.slabs:
            s.populations(f, g, fab)
        return f, g

    def LBM_hydrovars_density(self):
        return self._gather(NHYDROBAR, lambda s, o, fab: s.LBM_hydrovars_density(o, fab))

    def LBM_hydrovars(self, ncomp=NHYDRO):
        check(self.lib.bflbm_ring_prepare_ref(self._h))
        return self._gather(ncomp, lambda s, o, fab: s.LBM_hydrovars(o, fab, ncomp))

    def set_ref_state(self, rho_eq, phi_eq, rhot_eq, com_ref):
        n = self.n
        fab = make_fab((0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1))
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (rho_eq, phi_eq, rhot_eq)]
        check(self.lib.bflbm_ring_set_ref_state(self._h, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), ctypes.byref(fab)))
        c = (ctypes.c_double * 3)(*[float(v) for v in com_ref])
        check(self.lib.bflbm_ring_enable_ref_state(self._h, 1, c))

    def thermal_noise(self):
        check(self.lib.bflbm_ring_prepare_ref(self._h))
        fn = np.empty((NVEL, self.n[2], self.n[1], self.n[0])); gn = np.empty_like(fn)
        fab = make_fab((0, 0, 0), (self.n[0] - 1, self.n[1] - 1, self.n[2] - 1))
        for s in self.slabs:
            s.thermal_noise(fn, gn, fab)
        return fn, gn

    def update_com(self):
        s = (ctypes.c_double * 4)()
        check(self.lib.bflbm_ring_com_sums(self._h, s))
        s = np.array(list(s))
        return s[1:] / s[0]

    def mass(self):
        r, p = ctypes.c_double(), ctypes.c_double()
        check(self.lib.bflbm_ring_mass(self._h, ctypes.byref(r), ctypes.byref(p)))
        return r.value, p.value

    def sync(self):
        check(self.lib.bflbm_ring_sync(self._h))

    @property
    def steps_done(self):
        return self.slabs[0].steps_done

    def set_steps_done(self, n):
        check(self.lib.bflbm_ring_set_step_count(self._h, int(n)))

    TRANSPORTS = {"kernel": 0, "copy": 1}

    def set_transport(self, transport):
        """How the faces move: "kernel" (default) = one gather kernel per face reading the neighbour's planes in place
        (peer memory over xGMI); "copy" = the copy engine, 38 hipMemcpyPeerAsync per face, no compute units."""
        check(self.lib.bflbm_ring_set_transport(self._h, int(self.TRANSPORTS.get(transport, transport))))

    def set_overlap(self, on):
        """False: the faces move after the interior sweep instead of behind it (measures what the overlap buys)."""
        check(self.lib.bflbm_ring_set_overlap(self._h, 1 if on else 0))

    def last_transport(self):
        """(faces moved by the gather kernel, faces moved by the copy engine) in the last exchange."""
        a, b = ctypes.c_int(), ctypes.c_int()
        check(self.lib.bflbm_ring_last_transport(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


class BatchLBM:
    """B independent periodic lattices of one shape on one GPU, advanced by one launch per pass (bflbm_batch_*).

    params: one dict of model parameters (with replicas=B: replica r gets seed + r, or seeds[r]) or a list of B dicts
    (every field may differ, kBT included: all zero or all non-zero).  .replicas are borrowed BinaryLBM views: init,
    upload, observe, set_params and set_steps_done work on them as on a lone lattice; stepping goes through the batch.
    Each replica computes, bit for bit, what a lone BinaryLBM with the same parameters, state, step counter and exact
    schedule computes."""

    def __init__(self, n, params=None, replicas=None, seeds=None, device=0, schedule=None):
        self.lib = _lib.load()
        n = (n, n, n) if np.isscalar(n) else tuple(n)
        if len(n) != 3:
            raise ValueError("n: one size or three (nx, ny, nz)")
        self.n = tuple(int(v) for v in n)
        if params is None or isinstance(params, dict):
            if replicas is None:
                raise ValueError("BatchLBM: give replicas= with a single params dict")
            base = dict(params or {})
            seed0 = base.pop("seed", int(default_params().seed))
            if seeds is None:
                seeds = [seed0 + r for r in range(int(replicas))]
            plist = [dict(base, seed=int(seeds[r])) for r in range(int(replicas))]
        else:
            plist = [dict(p) for p in params]
            if replicas is not None and int(replicas) != len(plist):
                raise ValueError(f"BatchLBM: {len(plist)} parameter sets for replicas={replicas}")
            if seeds is not None:
                plist = [dict(p, seed=int(s)) for p, s in zip(plist, seeds)]
        if seeds is not None and len(seeds) != len(plist):
            raise ValueError("BatchLBM: one seed per replica")
        self.params = [default_params(**p) for p in plist]
        arr = (Params * max(1, len(self.params)))(*self.params)
        n3 = (ctypes.c_int * 3)(*self.n)
        h = ctypes.c_void_p()
        check(self.lib.bflbm_batch_create(arr, len(self.params), n3, int(device), ctypes.byref(h)))
        self._h = h
        self.replicas = []
        for r in range(len(self.params)):
            c = ctypes.c_void_p()
            check(self.lib.bflbm_batch_replica(self._h, r, ctypes.byref(c)))
            self.replicas.append(BinaryLBM._borrow(c, self.n, 0, self.n[2], 0, 1, self.params[r]))
        if schedule is not None:
            self.set_schedule(schedule)

    def __len__(self):
        return len(self.replicas)

    def close(self):
        if getattr(self, "_h", None):
            for d in list(getattr(self, "_dependents", [])):      # the batch's trace: closed; its structure-factor
                getattr(d, "_owner_closing", d.close)()           # accumulators: detached by the library, still readable
            for s in self.replicas:
                for d in list(getattr(s, "_dependents", [])):
                    d.close()
            self.lib.bflbm_batch_destroy(self._h)
            self._h = None
            for s in self.replicas:
                s._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_schedule(self, schedule):
        """"two_pass" (0), "fused" (1) or "auto" (2); the hand-over schedule is not available for batches."""
        check(self.lib.bflbm_batch_set_schedule(self._h, int(SCHEDULES.get(schedule, schedule))))

    def resolved_schedule(self):
        v = ctypes.c_int()
        check(self.lib.bflbm_batch_resolved_schedule(self._h, ctypes.byref(v)))
        return {0: "two_pass", 1: "fused"}[v.value]

    def LBM_timestep(self, nsteps=1):
        """LBM_timestep x nsteps on every replica."""
        check(self.lib.bflbm_batch_step(self._h, int(nsteps)))

    def sync(self):
        check(self.lib.bflbm_batch_sync(self._h))

    def trace(self, every, capacity, threshold=None):
        """Record every replica's droplet moments (cells with rho > threshold; None: every cell) after every `every`-th
        batch step."""
        return Trace(self, "bflbm_batch_trace_create", every, capacity, threshold)

    def interface_trace(self, level, field="rho", window=None, every=1, capacity=64):
        """Record every replica's contour heights (BinaryLBM.interface_trace) after every `every`-th batch step.  The
        device buffer is allocated at once: capacity x B x 2 ny nx doubles (the default 64 takes 32 MiB for 16 replicas
        of 8 x 256 columns)."""
        return InterfaceTrace(self, "bflbm_batch_iface_create", level, field, window, every, capacity)

    def shape_trace(self, level, nodes=None, field="rho", direction="falling", centre=None, threshold=None, step=0.5, rmax=None, every=1, capacity=64):
        """Record every replica's droplet radii along fixed rays (BinaryLBM.shape_trace) after every `every`-th batch step;
        a fixed centre is one for all replicas, the centre of mass is each replica's own."""
        return ShapeTrace(self, "bflbm_batch_shape_create", level, nodes, field, direction, centre, threshold, step, rmax, every, capacity)

    def spectrum_trace(self, var_names_or_pairs, kind="shell", every=1, capacity=64, lb_hydrovars=False, zero_avg=True, var_scaling=None):
        """Record every replica's binned structure factors (BinaryLBM.spectrum_trace) after every `every`-th batch step,
        with one observation launch, one batched transform and two binning launches per sample."""
        return SpectrumTrace(self, "bflbm_batch_spectrum_create", var_names_or_pairs, kind, every, capacity, lb_hydrovars, zero_avg, var_scaling)

    def mode_trace(self, variables, modes, every=1, capacity=64, lb_hydrovars=False):
        """Record every replica's Fourier amplitudes (BinaryLBM.mode_trace) after every `every`-th batch step, with one
        observation launch, one projection launch and one finishing launch per sample."""
        return ModeTrace(self, "bflbm_batch_modes_create", variables, modes, every, capacity, lb_hydrovars)

    def field_stats(self, variables, pairs=(), source="hydrovs", every=0):
        """Every replica's per-site means and covariances over frames (BinaryLBM.field_stats), with one observation launch
        and one accumulation launch per frame; replica=-1 reads the ensemble values.  No "noise" source on a batch."""
        return FieldStats(self, "bflbm_batch_fstat_create", variables, pairs, source, every)

    def profile_trace(self, variables, pairs=(), axis="z", source="hydrovs", every=1, capacity=64):
        """Every replica's plane sums along one axis (BinaryLBM.profile_trace) after every `every`-th batch step, with one
        observation launch, one plane launch and one finishing launch per sample."""
        return ProfileTrace(self, "bflbm_batch_profile_create", variables, pairs, axis, source, every, capacity)

    def histogram_trace(self, ranges, pairs=(), source="hydrovs", every=1, capacity=64):
        """Every replica's bin counts (BinaryLBM.histogram_trace) after every `every`-th batch step, with one counting
        launch over all replicas; the noise source is not available on a batch."""
        return HistogramTrace(self, "bflbm_batch_hist_create", ranges, pairs, source, every, capacity)

    def morphology_trace(self, variable, levels, side="above", source="hydrovs", every=1, capacity=64):
        """Every replica's cubes, faces, edges and vertices of a thresholded variable (BinaryLBM.morphology_trace) after
        every `every`-th batch step, with one observation launch, one counting launch over all replicas and one finishing
        launch per sample."""
        return MorphologyTrace(self, "bflbm_batch_morph_create", variable, levels, side, source, every, capacity)

    def chord_trace(self, variable, levels, side="above", max_length=64, source="hydrovs", every=1, capacity=64):
        """Every replica's chord-length distributions along x, y and z of a thresholded variable (BinaryLBM.chord_trace)
        after every `every`-th batch step: ChordTrace."""
        return ChordTrace(self, "bflbm_batch_chord_create", variable, levels, side, max_length, source, every, capacity)

    def coarse_trace(self, variables, pairs=(), block=(1, 1, 1), origin=(0, 0, 0), extent=None, source="hydrovs", every=1, capacity=64):
        """Every replica's block sums over a window (BinaryLBM.coarse_trace) after every `every`-th batch step, with one
        observation launch and one summing launch over all replicas per sample: CoarseTrace."""
        return CoarseTrace(self, "bflbm_batch_coarse_create", variables, pairs, block, origin, extent, source, every, capacity)

    def lag_trace(self, variables, pairs, origins=8, origin_stride=1, persist=None, source="hydrovs", every=1, capacity=64):
        """Every replica's two-time correlations against origins kept on the device (BinaryLBM.lag_trace) after every
        `every`-th batch step, with one observation launch and one summing launch over all replicas per sample; an
        origin carries each replica's own step counter: LagTrace."""
        return LagTrace(self, "bflbm_batch_lag_create", variables, pairs, origins, origin_stride, persist, source, every, capacity)

    def moment_trace(self, every=1, capacity=64):
        """Every replica's box sums of the 19 kinetic moments of both fluids, their squares and cross products
        (BinaryLBM.moment_trace) after every `every`-th batch step, with one summing launch over all replicas and one
        finishing launch per sample: MomentTrace."""
        return MomentTrace(self, "bflbm_batch_moment_create", every, capacity)

    def cluster_trace(self, variable, levels, side="above", connectivity=26, source="hydrovs", every=1, capacity=64):
        """Every replica's connected components of a thresholded variable (BinaryLBM.cluster_trace) after every `every`-th
        batch step, with one observation launch, four launches per level over all replicas and one finishing launch per
        sample."""
        return ClusterTrace(self, "bflbm_batch_cluster_create", variable, levels, side, connectivity, source, every, capacity)

    def component_trace(self, variable, levels, side="above", connectivity=26, min_size=1, rows=64, source="hydrovs", every=1, capacity=64):
        """Every replica's components one by one (BinaryLBM.component_trace) after every `every`-th batch step: ComponentTrace, whose record tabulates, per level, the `rows` components of at least `min_size` sites with
        the smallest labels: size, origin, extent, integer moments and area of each."""
        return ComponentTrace(self, "bflbm_batch_component_create", variable, levels, side, connectivity, min_size, rows, source, every, capacity)

    def radial_trace(self, variables, pairs=(), radials=(), centre=None, threshold=None, delta=1.0, nbins=None, source="hydrovs",
                     every=1, capacity=64):
        """Every replica's shell sums about its own centre of mass, or about one fixed centre (BinaryLBM.radial_trace), after
        every `every`-th batch step, with one observation launch, the two centre launches, one shell launch and one
        finishing launch per sample."""
        return RadialTrace(self, "bflbm_batch_radial_create", variables, pairs, radials, centre, threshold, delta, nbins, source, every, capacity)

    def structfact(self, var_names, **kw):
        """One structure-factor accumulator for the whole batch (structfact.BatchStructFact; every=k attaches it)."""
        from .structfact import BatchStructFact
        return BatchStructFact(self, var_names, **kw)

    # -- stacked getters: a leading replica axis ------------------------------------------------
    def populations(self):
        f = np.empty((len(self.replicas), NVEL, self.n[2], self.n[1], self.n[0]))
        g = np.empty_like(f)
        for r, s in enumerate(self.replicas):
            s.populations(f[r], g[r])
        return f, g

    def LBM_hydrovars(self, ncomp=NHYDRO):
        """hydrovs of every replica with one launch and one copy (bflbm_batch_get_hydrovs)."""
        out = np.empty((len(self.replicas), int(ncomp), self.n[2], self.n[1], self.n[0]))
        check(self.lib.bflbm_batch_get_hydrovs(self._h, _ptr(out), int(ncomp)))
        return out

    def LBM_hydrovars_density(self, ncomp=NHYDROBAR):
        """hydrovsbar of every replica with one launch and one copy (bflbm_batch_get_hydrovsbar)."""
        out = np.empty((len(self.replicas), int(ncomp), self.n[2], self.n[1], self.n[0]))
        check(self.lib.bflbm_batch_get_hydrovsbar(self._h, _ptr(out), int(ncomp)))
        return out


PLAN_FIELDS = ("tile_x", "tile_y", "ntx", "nty", "sx", "planes_per_chunk", "chunks", "last_chunk_planes",
               "workgroups_per_replica", "workgroups", "rounds", "per_xcd", "grid", "compute_units")


def fused_plan_query(n, replicas=1, noise=False, compute_units=0):
    """The launch plan of the one-pass schedule for a lattice n = (nx, ny, nz): a lone lattice (replicas=1) or a batch,
    from the library's own planner (bflbm_fused_plan_query; no device needed).  compute_units=0: the device's count once
    a context exists, 256 before.  -> dict of PLAN_FIELDS."""
    n = (n, n, n) if np.isscalar(n) else tuple(n)
    n3 = (ctypes.c_int * 3)(*[int(v) for v in n])
    out = (ctypes.c_int * 16)()
    check(_lib.load().bflbm_fused_plan_query(n3, int(replicas), int(bool(noise)), int(compute_units), out))
    return dict(zip(PLAN_FIELDS, list(out)))


SWEEP_PLAN_FIELDS = ("tile_x", "tile_y", "ntx", "nty", "sx", "planes_per_chunk", "chunks", "last_chunk_planes", "chunk_stride",
                     "workgroups", "rounds", "per_xcd", "grid", "compute_units", "pair_planes", "pair_stride")


def sweep_plan_query(n, schedule="handover", noise=False, slab_planes=0, compute_units=0):
    """The launch plans of the plane-marching sweeps of one step of a lone context (bflbm_sweep_plan_query; no device
    needed): schedule "fused" or "handover"; slab_planes=0 the whole periodic lattice n, otherwise the interior sweep of a
    ring's slab of that many planes and its boundary-pair launch.  compute_units as in fused_plan_query.
    -> dict of SWEEP_PLAN_FIELDS."""
    n = (n, n, n) if np.isscalar(n) else tuple(n)
    n3 = (ctypes.c_int * 3)(*[int(v) for v in n])
    out = (ctypes.c_int * 16)()
    check(_lib.load().bflbm_sweep_plan_query(n3, int(SCHEDULES.get(schedule, schedule)), int(bool(noise)), int(slab_planes),
                                             int(compute_units), out))
    return dict(zip(SWEEP_PLAN_FIELDS, list(out)))


def rng_site_normals(seed, site, noise_index):
    """Host evaluation of the project's Gaussian stream: the 33 normals of one site and noise index."""
    out = (ctypes.c_double * 36)()
    check(_lib.load().bflbm_rng_site_normals(int(seed), int(site), int(noise_index), out))
    return np.array(list(out))[:33]
