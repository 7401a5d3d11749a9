"""An independent numpy restatement of the BSDF query (tor_bsdf_eval_device), written from the text of include/tor_bsdf.h, not from
the kernel: elementwise float64 operations over all items, in the header's order -- numpy's float64 `+ - * /` and sqrt are single
IEEE roundings and never fuse.  It shares no code with the library.  tests/test_bsdf_query.py shows that what it states IS the
density of the reference's scatter (bounce_restatement.scatter over the oracle's generator); tests/test_gpu_bsdf_query.py holds
the kernel to it bit for bit.  Records are the flat (n, 16) {kind, c0 xyz, c1 xyz, t0, t1, radius, material, albedo rgb, fuzz, ri}
of Scene.from_records; hit records the (n, 8) words of hit_restatement.world_hit."""
import numpy as np

NONE, DENSITY, DELTA = 0, 1, 2
LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2
PI = 3.141592653589793


def _dot(u, v):
    """vec3s.nim:96-98, from the left."""
    return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]


def _listed(index, n):
    if index is None:
        return np.arange(n)
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    return index[(index >= 0) & (index < n)]                              # entries outside [0, n) are skipped


def metal_density(w, d_in, nrm, fuzz):
    """tor_bsdf.h "Metal" for unit rows w: the density of unit(r + f B) at w, r = reflect(unit(d_in), nrm)."""
    with np.errstate(all="ignore"):
        ud = d_in * (1.0 / np.sqrt(_dot(d_in, d_in)))[:, None]
        r = ud - nrm * (2.0 * _dot(ud, nrm))[:, None]
        f = np.abs(fuzz)
        b = _dot(w, r)
        x = np.stack([w[:, 1] * r[:, 2] - w[:, 2] * r[:, 1], w[:, 2] * r[:, 0] - w[:, 0] * r[:, 2],
                      w[:, 0] * r[:, 1] - w[:, 1] * r[:, 0]], axis=1)
        s2 = _dot(x, x)
        h = f * f - s2
        q = np.sqrt(h)
        lo, hi = b - q, b + q
        f3 = f * f * f
        outer = (q * (3.0 * b * b + h)) / (2.0 * PI * f3)
        holds = (hi * hi * hi) / (4.0 * PI * f3)
        return np.where(h > 0, np.where(lo > 0, outer, np.where(hi > 0, holds, 0.0)), 0.0)


def evaluate(recs, rays_in, raw, rays_out, index=None, out=None):
    """tor_bsdf_eval_device for the listed items: a dict of value (n, 3), pdf (n,) and kind (n,) int32; items that are not listed
    keep what `out` (an earlier result) holds, else 0."""
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, 16)
    rays_in = np.asarray(rays_in, dtype=np.float64).reshape(-1, 7)
    rays_out = np.asarray(rays_out, dtype=np.float64).reshape(-1, 7)
    raw = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1, 8)
    n = rays_in.shape[0]
    value = np.zeros((n, 3)) if out is None else out["value"]
    pdf = np.zeros(n) if out is None else out["pdf"]
    kind = np.zeros(n, dtype=np.int32) if out is None else out["kind"]
    ids = _listed(index, n)
    obj = raw.view(np.int32)[ids, 14].astype(np.int64)
    known = (obj >= 0) & (obj < recs.shape[0])
    value[ids[~known]], pdf[ids[~known]], kind[ids[~known]] = 0.0, 0.0, NONE
    ids, obj = ids[known], obj[known]
    o = recs[obj]
    mat, fuzz, albedo = o[:, 10].astype(np.int64), o[:, 14], o[:, 11:14]
    dense = (mat == LAMBERTIAN) | ((mat == METAL) & (fuzz != 0.0))
    value[ids[~dense]], pdf[ids[~dense]], kind[ids[~dense]] = 0.0, 0.0, DELTA
    ids, mat, fuzz, albedo = ids[dense], mat[dense], fuzz[dense], albedo[dense]
    d_in, nrm, d_out = rays_in[ids, 3:6], raw[ids, 3:6], rays_out[ids, 3:6]
    with np.errstate(all="ignore"):
        oo = _dot(d_out, d_out)
        usable = (oo > 0) & (oo < np.inf)
        w = d_out * (1.0 / np.sqrt(oo))[:, None]
        gate = _dot(d_out, nrm) > 0
        c = _dot(w, nrm)
        lam = np.where(c > 0, c / PI, 0.0)
        met = metal_density(w, d_in, nrm, fuzz)
        p = np.where(usable & gate, np.where(mat == LAMBERTIAN, lam, met), 0.0)
        value[ids], pdf[ids], kind[ids] = albedo * p[:, None], p, DENSITY
    return {"value": value, "pdf": pdf, "kind": kind}


def same_bits(got, want):
    """Elementwise: equal in every bit, or NaN on both sides (a NaN's sign and payload are not defined, tor_bsdf.h)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
