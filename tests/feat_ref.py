"""Plain numpy restatement of the scan feature extraction.

Written from the survey's description of calculateSmoothness / markOccludedPoints / extractFeatures, independent of the
C++ oracle and of the HIP kernels.  Where the reference leaves something open this file fixes it, and the GPU tests pin
the HIP library to exactly this:

* the sort of a sector's `cloudSmoothness[sp, ep)` is a TOTAL order, ascending (value, ind).  The corner walk goes down
  the sorted range, so among equal curvatures the larger index comes first; the surf walk goes up, so the smaller index
  comes first.  Slot `ep` lies outside the sorted range: first in the corner walk, last in the surf walk.
* the neighbour marks stop at the cloud's ends (indices < 0 or >= n) as at a column jump above 10.

State persists across scans as in the node: the four arrays are zero-initialised once and only [5, n-5) is rewritten per
scan.  What survives and matters is slot 4 of cloudSmoothness, never rewritten = {0, ind 0}: whichever ring's sector 0
starts at 4 sorts it in.  Under the total order it stays the smallest entry, so it stays in slot 4; the surf walk visits it
first and, as long as picked[0] is still 0, labels ind 0 and marks picked[1..5] (up to a column jump)."""
import numpy as np

CORNER_CAP = 40


def cdiv(a, b):
    """C integer division (truncates towards zero)"""
    q = abs(a) // b
    return q if a >= 0 else -q


def sector_bounds(start, end, j):
    sp = cdiv(start * (6 - j) + end * j, 6)
    ep = cdiv(start * (5 - j) + end * (j + 1), 6) - 1
    return sp, ep


def curvature(r):
    """a-1 for i in [5, n-5): float32, one rounding per operation, left to right"""
    r = np.asarray(r, np.float32)
    n = len(r)
    if n <= 10:
        return np.zeros(0, np.float32)
    c = r[5:n - 5]
    d = (r[3:n - 7] + r[4:n - 6]) - c * np.float32(4)
    d = d + r[6:n - 4]
    d = d + r[7:n - 3]
    assert d.dtype == np.float32
    return d * d


class FeatRef:
    def __init__(self, N_SCAN, Horizon_SCAN, edgeThreshold, surfThreshold):
        full = int(N_SCAN) * int(Horizon_SCAN)
        self.N_SCAN = int(N_SCAN)
        self.edge, self.surf = np.float32(edgeThreshold), np.float32(surfThreshold)
        self.curv = np.zeros(full, np.float32)
        self.picked = np.zeros(full, np.int32)
        self.label = np.zeros(full, np.int32)
        self.sm_val = np.zeros(full, np.float32)
        self.sm_ind = np.zeros(full, np.int64)

    # ---- a-1
    def _smoothness(self, r):
        n = len(r)
        if n <= 10:
            return
        w = slice(5, n - 5)
        self.curv[w] = curvature(r)
        self.picked[w] = 0
        self.label[w] = 0
        self.sm_val[w] = self.curv[w]
        self.sm_ind[w] = np.arange(5, n - 5)

    # ---- a-2
    def _occlusion(self, r, col):
        n = len(r)
        if n - 6 <= 5:
            return
        i = np.arange(5, n - 6)
        near = np.abs(col[i + 1] - col[i]) < 10
        d12 = (r[i] - r[i + 1]).astype(np.float64)          # float32 difference, compared as double
        d21 = (r[i + 1] - r[i]).astype(np.float64)
        a = near & (d12 > 0.3)
        b = near & ~(d12 > 0.3) & (d21 > 0.3)
        self.picked[i[a] - 1] = 1
        self.picked[i[a]] = 1
        self.picked[i[b] + 1] = 1
        self.picked[i[b] + 2] = 1
        diff1 = np.abs(r[i - 1] - r[i]).astype(np.float64)
        diff2 = np.abs(r[i + 1] - r[i]).astype(np.float64)
        lim = 0.1 * r[i].astype(np.float64)                 # double product
        self.picked[i[(diff1 > lim) & (diff2 > lim)]] = 1

    def _mark(self, ind, col, n):
        self.picked[ind] = 1
        for l in range(1, 6):
            k = ind + l
            if k >= n or abs(int(col[k]) - int(col[k - 1])) > 10:
                break
            self.picked[k] = 1
        for l in range(1, 6):
            k = ind - l
            if k < 0 or abs(int(col[k]) - int(col[k + 1])) > 10:
                break
            self.picked[k] = 1

    def extract(self, point_range, point_col_ind, start_ring_index, end_ring_index):
        r = np.ascontiguousarray(point_range, np.float32)
        col = np.ascontiguousarray(point_col_ind, np.int64)
        n = len(r)
        self._smoothness(r)
        self._occlusion(r, col)
        occl = self.picked[:n].copy()
        corners, sectors = [], []
        for ring in range(self.N_SCAN):
            for j in range(6):
                sp, ep = sector_bounds(int(start_ring_index[ring]), int(end_ring_index[ring]), j)
                if sp >= ep:
                    continue
                order = np.lexsort((self.sm_ind[sp:ep], self.sm_val[sp:ep]))         # ascending (value, ind)
                self.sm_val[sp:ep] = self.sm_val[sp:ep][order]
                self.sm_ind[sp:ep] = self.sm_ind[sp:ep][order]
                inds = self.sm_ind[sp:ep + 1]
                # candidates of the sorted range as the sector finds them, from the top (slot ep is not among them)
                desc = inds[:-1][::-1]
                cand = [int(i) for i in desc if self.picked[i] == 0 and self.curv[i] > self.edge]
                rank_of = {i: q for q, i in enumerate(cand)}
                taken, ranks, n_elig, broke = [], [], 0, False
                for k in range(ep, sp - 1, -1):
                    ind = int(self.sm_ind[k])
                    if self.picked[ind] == 0 and self.curv[ind] > self.edge:
                        n_elig += 1
                        if n_elig > CORNER_CAP:
                            broke = True                 # the 41st eligible point: break, nothing marked
                            break
                        self.label[ind] = 1
                        taken.append(ind)
                        ranks.append(rank_of.get(ind, -1))           # -1: the ep slot
                        self._mark(ind, col, n)
                for k in range(sp, ep + 1):
                    ind = int(self.sm_ind[k])
                    if self.picked[ind] == 0 and self.curv[ind] < self.surf:
                        self.label[ind] = -1
                        self._mark(ind, col, n)
                corners += taken
                sectors.append(dict(ring=ring, sec=j, sp=sp, ep=ep, cand=cand, taken=taken, ranks=ranks, broke=broke))
        return dict(n=n, curv=self.curv[:n].copy(), occl=occl, label=self.label[:n].copy(), picked=self.picked[:n].copy(),
                    corner_idx=np.asarray(corners, np.int32), sectors=sectors)
