"""Runs the reference's own compiled code (oracle/_ref/ref_main, built by oracle/ref_harness from the reference's headers
against amrex_lite.H) as a subprocess and returns its arrays.  Test infrastructure only.

Two binaries: `ref_main` (the reference as shipped) and `ref_main_refstate` (-DUSE_REF_STATE).  Requests and replies go
through files in a temporary directory; doubles cross the text request as C99 hex floats, i.e. exactly."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
Q = 19
RECORD = (("f", 19), ("g", 19), ("hbar", 15), ("h", 22), ("fn", 19), ("gn", 19))
MODEL_KEYS = ("tau_f", "tau_g", "alpha0", "alpha1", "kappa", "kBT")
DEFAULTS = dict(tau_f=0.5, tau_g=0.5, alpha0=4.0, alpha1=0.0, kappa=4.0, kBT=0.0)     # LBM_binary.H:18-30, LBM_d3q19.H:10


def binary(ref_state=False):
    return os.path.join(REF_DIR, "ref_main_refstate" if ref_state else "ref_main")


def available():
    return all(os.access(binary(r), os.X_OK) for r in (False, True))


def build_info():
    path = os.path.join(REF_DIR, "BUILD_INFO")
    return open(path).read().strip().splitlines() if os.path.exists(path) else ["unknown", "unknown"]


def _hex(v):
    return float(v).hex()


def _vec(v):
    return " ".join(_hex(x) for x in v)


def _call(lines, files, n, ref_state, nout):
    """lines: request lines; files: {key: array} written as raw doubles and named in the request."""
    with tempfile.TemporaryDirectory(prefix="bflbm_ref_") as tmp:
        out = os.path.join(tmp, "out.bin")
        lines = list(lines) + ["n %d %d %d" % tuple(n), "out " + out]
        for key, arr in files.items():
            path = os.path.join(tmp, key + ".bin")
            np.ascontiguousarray(arr, dtype="<f8").tofile(path)
            lines.append(f"{key} {path}")
        req = os.path.join(tmp, "request.txt")
        with open(req, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        p = subprocess.run([binary(ref_state), req], capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"reference binary failed ({p.returncode}): {p.stderr.strip()}")
        data = np.fromfile(out, dtype="<f8")
    if data.size != nout:
        raise RuntimeError(f"reference binary wrote {data.size} doubles, expected {nout}")
    return data, p.stdout


def _model(par):
    unknown = set(par) - set(MODEL_KEYS)
    if unknown:
        raise KeyError(f"not a mutable global of the reference: {sorted(unknown)}")
    full = dict(DEFAULTS, **par)
    return [f"{k} {_hex(full[k])}" for k in MODEL_KEYS]


def _ref_lines(files, refstate, com, com_ref):
    lines = []
    if refstate is not None:
        files["refstate"] = np.stack([np.asarray(a, dtype=np.float64) for a in refstate])
    for c in ([] if com is None else np.atleast_2d(np.asarray(com, dtype=np.float64))):
        lines.append("com " + _vec(c))
    if com_ref is not None:
        lines.append("com_ref " + _vec(com_ref))
    return lines


def run(n, par, init, steps, dump, normals=None, refstate=None, com=None, com_ref=None, stdout=False):
    """LBM_init_* then `steps` x LBM_timestep.  init: ("stripe", frac) | ("droplet", r) | ("mixture",) | ("file", f0, g0).
    -> {step: {"f","g","hbar","h","fn","gn"}} for the steps in `dump`; arrays are (c, nz, ny, nx).
    normals: the table RandomNormal hands out, (steps + 1) x sites x 33 entries in the reference's call order.
    com: what update_com returns (one vector, or one per call); with refstate the USE_REF_STATE binary runs."""
    nx, ny, nz = n
    ns = nx * ny * nz
    dump = sorted(set(int(s) for s in dump))
    assert dump and dump[-1] <= steps
    files = {}
    lines = ["mode run"] + _model(par) + [f"steps {int(steps)}", "dump " + " ".join(map(str, dump))]
    if init[0] == "file":
        files["state"] = np.stack([np.asarray(init[1], dtype=np.float64), np.asarray(init[2], dtype=np.float64)])
        lines.append("init file")
    elif init[0] == "mixture":
        lines.append("init mixture")
    else:
        lines.append(f"init {init[0]} {_hex(init[1])}")
    if normals is not None:
        files["normals"] = normals
    lines += _ref_lines(files, refstate, com, com_ref)
    per = sum(c for _, c in RECORD) * ns
    data, text = _call(lines, files, n, refstate is not None, per * len(dump))
    out = {}
    for i, s in enumerate(dump):
        rec, o = {}, i * per
        for name, c in RECORD:
            rec[name] = data[o:o + c * ns].reshape(c, nz, ny, nx).copy()
            o += c * ns
        out[s] = rec
    return (out, text) if stdout else out


def thermal_noise(n, par, rho, phi, normals, refstate=None, shift=(0.0, 0.0, 0.0)):
    """thermal_noise (LBM_binary.H:73-132) alone, on hydrovsbar comps 0, 1 = rho, phi; with refstate = (rho_eq, phi_eq,
    rhot_eq) the USE_REF_STATE binary reads those at the site shifted by trunc(shift).  -> fn, gn (19, nz, ny, nx)."""
    nx, ny, nz = n
    ns = nx * ny * nz
    files = {"hbar": np.stack([np.asarray(rho, dtype=np.float64), np.asarray(phi, dtype=np.float64)]), "normals": normals}
    lines = ["mode noise"] + _model(par) + ["shift " + _vec(shift)] + _ref_lines(files, refstate, None, None)
    data, _ = _call(lines, files, n, refstate is not None, 2 * Q * ns)
    return data[:Q * ns].reshape(Q, nz, ny, nx).copy(), data[Q * ns:].reshape(Q, nz, ny, nx).copy()


def units(vec, fields, u, a, field, tau_f=0.5):
    """The site functions of SURVEY 8c's list on supplied inputs: vec (K, 19), fields (K, 2), u (K, 3), a (K, 3) and one
    scalar field (nz, ny, nx) with periodic images.  -> dict of moments, populations, equilibrium_moments[index],
    phi_moments[index] (K, 19 each), gradient and grad_laplacian_2nd (3, nz, ny, nx)."""
    K = len(vec)
    nz, ny, nx = field.shape
    ns = nx * ny * nz
    blob = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in (vec, fields, u, a, field)])
    lines = ["mode unit"] + _model(dict(tau_f=tau_f)) + [f"count {K}"]
    data, _ = _call(lines, {"unit": blob}, (nx, ny, nz), False, 6 * K * Q + 6 * ns)
    names = ("moments", "populations", "equilibrium_moments_0", "equilibrium_moments_1", "phi_moments_0", "phi_moments_1")
    out = {nm: data[i * K * Q:(i + 1) * K * Q].reshape(K, Q).copy() for i, nm in enumerate(names)}
    o = 6 * K * Q
    out["gradient"] = data[o:o + 3 * ns].reshape(3, nz, ny, nx).copy()
    out["grad_laplacian_2nd"] = data[o + 3 * ns:].reshape(3, nz, ny, nx).copy()
    return out


def reference_order(z33):
    """The project's 33 normals of a site (3 momentum, 15 of f, 15 of g: orc_site_normals) in the order the reference
    draws them (LBM_binary.H:115-127): modes 1..3, then (f_a, g_a) for a = 4..18."""
    z33 = np.asarray(z33)
    out = np.empty_like(z33)
    out[..., :3] = z33[..., :3]
    out[..., 3::2] = z33[..., 3:18]
    out[..., 4::2] = z33[..., 18:33]
    return out
