"""The checker of temporal reprojection: tests/temporal_oracle.c compiled with the CFLAGS of oracle/Makefile and bound with ctypes, a
lock-step driver that holds the checker's own state from call 0, a float64 numpy restatement of the same definition written from the
text of include/rt.h, and the cameras the temporal tests share.  Test infrastructure only."""
import ctypes

import numpy as np

from checker_build import compile_checker

DEFAULTS = dict(maxHistory=32, depthTolerance=0.05, normalTolerance=0.5)        # RT_TEMPORAL_DEFAULT_* of include/rt.h
TIGHT = dict(depthTolerance=0.01, normalTolerance=0.1)
WIDE = dict(depthTolerance=0.6, normalTolerance=2.0)

_lib = None


def shim():
    global _lib
    if _lib is None:
        lib = compile_checker("temporal_oracle.c")
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        lib.temporal_step.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, cf, cf, ci, vp, vp, vp, vp]
        lib.temporal_step.restype = ci
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def camera_of(params):
    """(M[16], O[3], V[3]) float32: the camera fields of an rt_params record (or of a mapping with the same keys)"""
    return (np.ascontiguousarray(params["camLocalToWorld"], np.float32).reshape(16).copy(),
            np.ascontiguousarray(params["worldSpaceCameraPos"], np.float32).reshape(3).copy(),
            np.ascontiguousarray(params["viewParams"], np.float32).reshape(3).copy())


def rigid_camera(position, yaw=0.0, pitch=0.0, roll=0.0, view=(1.2, 0.8, 1.0)):
    """the camera fields of a rigid pose: rotation = yaw about y, then pitch about x, then roll about z; columns right, up, forward"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Ry @ Rx @ Rz
    M[:3, 3] = position
    return {"camLocalToWorld": M.astype(np.float32).reshape(16), "worldSpaceCameraPos": np.asarray(position, np.float32),
            "viewParams": np.asarray(view, np.float32)}


def random_camera_pair(seed, step=0.05, turn=0.02):
    """two rigid poses a small random motion apart (position within the unit cube, any heading)"""
    rng = np.random.default_rng(seed)
    pos, ang = rng.uniform(-1, 1, 3), rng.uniform(-np.pi, np.pi, 3) * (1.0, 0.3, 0.3)
    view = (float(rng.uniform(0.8, 1.6)), float(rng.uniform(0.6, 1.2)), 1.0)
    a = rigid_camera(pos, *ang, view=view)
    b = rigid_camera(pos + rng.uniform(-step, step, 3), *(ang + rng.uniform(-turn, turn, 3)), view=view)
    return a, b


class Checker:
    """The lock-step driver: the C checker's own T, N, G' and previous camera from call 0.  step() is one rt_temporal call."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.T = self.N = self.G = self.cam = self.code = None
        self.calls = 0

    def step(self, C, A, G, camera, maxHistory=32, depthTolerance=0.05, normalTolerance=0.5, variant=0):
        C, A, G = (np.ascontiguousarray(a, np.float32) for a in (C, A, G))
        assert C.shape == A.shape == G.shape and C.ndim == 3 and C.shape[2] == 4
        H, W = C.shape[:2]
        if self.T is not None and self.T.shape != C.shape:
            self.reset()                                       # a size change drops the history
        cam = camera_of(camera)
        have = self.T is not None
        Tp, Np, Gp = (self.T, self.N, self.G) if have else (np.zeros_like(C), np.zeros((H, W), np.float32), np.zeros_like(C))
        Mp, Op, Vp = self.cam if have else cam
        T, N, Gn, code = np.empty_like(C), np.empty((H, W), np.float32), np.empty_like(C), np.empty((H, W, 3), np.int32)
        rc = shim().temporal_step(_p(C), _p(A), _p(G), W, H, _p(cam[0]), _p(cam[1]), _p(cam[2]), _p(Mp), _p(Op), _p(Vp),
                                  _p(Tp), _p(Np), _p(Gp), 1 if have else 0, int(maxHistory), depthTolerance, normalTolerance, int(variant),
                                  _p(T), _p(N), _p(Gn), _p(code))
        assert rc == 0
        self.T, self.N, self.G, self.cam, self.code = T, N, Gn, cam, code
        self.calls += 1
        return T, N


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


class Twin64:
    """The definition in float64, written from the header's text, vectorised over the image.  Besides T and N a step leaves `code` (the
    decisions, in the checker's encoding), `sw` and `px_scale`: per pixel the factor that turns a relative rounding error of the
    reprojection chain into pixels (DESIGN.md "Temporal reprojection": the tolerance of the twin comparison)."""

    def __init__(self):
        self.T = self.N = self.G = self.cam = None

    def step(self, C, A, G, camera, maxHistory=32, depthTolerance=0.05, normalTolerance=0.5):
        C, A, G = (np.asarray(a, np.float32).astype(np.float64) for a in (C, A, G))
        H, W = C.shape[:2]
        M, O, V = (a.astype(np.float64) for a in camera_of(camera))
        dt, nt = float(np.float32(depthTolerance)), float(np.float32(normalTolerance))
        cov = A[..., 3]
        surf = cov > 0
        safe = np.where(surf, cov, 1.0)
        nc = np.where(surf[..., None], G[..., :3] / safe[..., None], 0.0)
        zc = np.where(surf, G[..., 3] / safe, 0.0)
        code = np.zeros((H, W, 3), np.int32)
        sw, hn, h = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, 3))
        self.px_scale = np.zeros((H, W))
        if self.T is not None:
            Mp, Op, Vp = self.cam
            ys, xs = np.mgrid[0:H, 0:W]
            lx, ly = ((xs + 0.5) / W - 0.5) * V[0], ((ys + 0.5) / H - 0.5) * V[1]
            l = np.stack([lx, ly, np.full_like(lx, V[2]), np.ones_like(lx)], -1)
            F = l @ M.reshape(4, 4)[:3].T
            d = F - O
            dirn = d / np.sqrt(_dot(d, d))[..., None]
            X = O + dirn * zc[..., None]
            tprev = Mp.reshape(4, 4)[:3, 3]
            q = np.where(surf[..., None], X - tprev, dirn)
            ze = np.sqrt(_dot(X - Op, X - Op))
            R = Mp.reshape(4, 4)[:3, :3]
            with np.errstate(all="ignore"):
                lp = np.stack([_dot(np.broadcast_to(R[:, i], q.shape), q) / (R[:, i] @ R[:, i]) for i in range(3)], -1)
                s = Vp[2] / lp[..., 2]
                px = (lp[..., 0] * s / Vp[0] + 0.5) * W - 0.5
                py = (lp[..., 1] * s / Vp[1] + 0.5) * H - 0.5
                valid = (lp[..., 2] > 0) & (px > -1) & (px < W) & (py > -1) & (py < H)
                # a relative error e of the chain moves px by at most e * px_scale pixels: the magnitudes that enter the sums
                # (|O| + |t'| + zc + focus distance) over the depth in the previous camera, times pixels per unit of l'_x / l'_z
                mag = np.abs(O).sum() + np.abs(tprev).sum() + np.abs(Op).sum() + zc + np.abs(V).sum()
                ratio = 1.0 + np.maximum(np.abs(lp[..., 0]), np.abs(lp[..., 1])) / np.abs(lp[..., 2])
                self.px_scale = np.where(valid, mag / np.abs(lp[..., 2]) * ratio * max(W / Vp[0], H / Vp[1]) * Vp[2], 0.0)
            x0 = np.where(valid, np.floor(np.where(valid, px, 0.0)), 0.0)
            y0 = np.where(valid, np.floor(np.where(valid, py, 0.0)), 0.0)
            fx, fy = px - x0, py - y0
            code[..., 0] = valid
            code[..., 1], code[..., 2] = x0, y0
            for j in (0, 1):
                for i in (0, 1):
                    tx, ty = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
                    inside = valid & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                    cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    Tq, Nq, Gq = self.T[cy, cx], self.N[cy, cx], self.G[cy, cx]
                    e = nc - Gq[..., :3]
                    with np.errstate(all="ignore"):
                        ok_surf = (Gq[..., 3] > 0) & (np.abs(Gq[..., 3] - ze) <= dt * ze) & (_dot(e, e) <= nt * nt)
                        counts = inside & (Nq > 0) & np.where(surf, ok_surf, Gq[..., 3] == 0)
                        b = np.where(counts, (fx if i else 1.0 - fx) * (fy if j else 1.0 - fy), 0.0)
                    code[..., 0] |= counts.astype(np.int32) * (2 << (j * 2 + i))
                    sw += b
                    h += b[..., None] * np.where(counts[..., None], Tq[..., :3], 0.0)
                    hn += b * np.where(counts, Nq, 0.0)
        hist = sw >= float(np.float32(0.01))
        ssw = np.where(hist, sw, 1.0)
        t = hn / ssw + 1.0
        n = np.where(hist, np.minimum(t, float(maxHistory)), 1.0)
        a = 1.0 / n
        T = np.empty_like(C)
        T[..., :3] = np.where(hist[..., None], (h / ssw[..., None]) * (1.0 - a)[..., None] + C[..., :3] * a[..., None], C[..., :3])
        T[..., 3] = C[..., 3]
        code[..., 0] |= hist.astype(np.int32) * 32 | (hist & ~(t < maxHistory)).astype(np.int32) * 64
        self.T, self.N, self.G, self.cam = T, n, np.concatenate([nc, zc[..., None]], -1), (M, O, V)
        self.code, self.sw = code, np.where(hist, sw, 0.0)
        return T, n


def posed(rtx, mgr, params, offset=(0.0, 0.0, 0.0), yaw=0.0):
    """a copy of `params` with the manager's camera moved by `offset` and turned by `yaw` about the world's y axis"""
    t = mgr.camera.transform
    position, rotation = np.array(t.position, np.float32), np.array(t.rotation, np.float32)
    try:
        t.position = position + np.asarray(offset, np.float32)
        t.rotation = rtx.host.quat_mul((0.0, float(np.sin(yaw / 2)), 0.0, float(np.cos(yaw / 2))), rotation)
        out = np.array(params, dtype=rtx.PARAMS).reshape(()).copy()
        mgr.UpdateCameraParams(out)
    finally:
        t.position, t.rotation = position, rotation
    return out
