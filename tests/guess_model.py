"""numpy model of ksp_guess_type fischer as oasisx_amd/ksp.py and csrc/ox_guess.hip run it (no GPU): per column an
A-orthonormal basis x~_j, stored as unscaled v_j with a scale sigma_j (0: a slot of the skip rule); model 1 also keeps
A v_j.  The same operations in the same order as the device, up to the summation order of the dot products."""
import numpy as np


class FischerModel:
    def __init__(self, A, nc: int = 1, model: int = 1, size: int = 10):
        self.A, self.nc, self.model, self.size = A, nc, model, size
        self.v, self.w, self.sigma = [], [], []  # per slot: (n, nc), (n, nc), (nc,)
        self.x0 = None

    @property
    def k(self) -> int:
        return len(self.v)

    def basis(self, c: int) -> np.ndarray:
        """(n, k) the x~_j of column c."""
        if not self.v:
            return np.zeros((self.A.shape[0], 0))
        return np.stack([s[c] * v[:, c] for v, s in zip(self.v, self.sigma)], axis=1)

    def form(self, b, xw=None, axw=None):
        """The initial guess (None while the basis is empty: the caller's solve as it stands).  xw: the warm start
        (None: zero)."""
        b = b.reshape(len(b), -1)
        self.x0 = None
        if self.k == 0:
            return None
        xw = np.zeros_like(b) if xw is None else xw.reshape(b.shape)
        axw = (self.A @ xw) if axw is None else axw.reshape(b.shape)
        r = b - axw
        x = xw.copy()
        for v, s in zip(self.v, self.sigma):
            x += v * (s * s * np.einsum("ic,ic->c", v, r))
        self.x0 = x.copy()
        return x

    def update(self, x):
        """After a converged solve: add d = x - x0 (d = x when the basis was empty or is restarted)."""
        x = x.reshape(x.shape[0], -1)
        if self.k == self.size:
            self.v, self.w, self.sigma = [], [], []
            self.x0 = None
        d = x - self.x0 if (self.x0 is not None and self.k > 0) else x.copy()
        self.x0 = None
        ad = self.A @ d
        pre = np.einsum("ic,ic->c", d, ad)
        if self.k:
            beta = [s * s * np.einsum("ic,ic->c", v, ad) for v, s in zip(self.v, self.sigma)]
            for v, bj in zip(self.v, beta):
                d = d - v * bj
            if self.model == 1:
                for w, bj in zip(self.w, beta):
                    ad = ad - w * bj
            else:
                ad = self.A @ d
            post = np.einsum("ic,ic->c", d, ad)
        else:
            post = pre
        ok = (pre > 0) & (post > 0) & (post > 1e-20 * pre)
        self.v.append(d)
        self.w.append(ad)
        self.sigma.append(np.where(ok, 1.0 / np.sqrt(np.where(ok, post, 1.0)), 0.0))


def projected_guess(A, X, b, xw):
    """x_w plus the A-orthogonal projection of the error onto span(X), from the Gram system (reference formula)."""
    if X.shape[1] == 0:
        return xw.copy()
    G = X.T @ (A @ X)
    alpha = np.linalg.solve(G, X.T @ (b - A @ xw))
    return xw + X @ alpha
