"""Float64 statement of dslam_register_graph: the joint alignment of N maps from a list of
overlapping pairs, in numpy, on maps given as ref64_register.MapData.  Every pair is evaluated by ref64_register.evaluate
(section 13's law with its rounding bound and ties); this file adds the pair transforms, the active pairs, the joint
cost, the pivots, the Jacobians, the reduced system, the acceptance, the stop reasons and the conditioning.  Shares no
text with the engine.

Poses.  T_i: world -> map i, 4 x 4 in metres, taken as float32 (the ABI's); T~_i: the first three rows in float64 with the
translation divided by the voxel size.  X~_p = T~_d inv(T~_s) with inv = (R^T, -(R^T t)) and every sum evaluated left to
right in Python floats (the mirror's RigidInverse / RigidProduct), not as a matrix product of numpy's.
"""
import numpy as np

import ref64_register as rr

DEFAULTS = rr.DEFAULTS


# ---------------------------------------------------------------------------------------------------------------------
# rigid 3 x 4 arithmetic in the stated scalar order
# ---------------------------------------------------------------------------------------------------------------------
def rigid_inverse(X):
    X = [[float(v) for v in row] for row in X]
    out = np.empty((3, 4))
    for r in range(3):
        for c in range(3):
            out[r, c] = X[c][r]
        out[r, 3] = -((X[0][r] * X[0][3] + X[1][r] * X[1][3]) + X[2][r] * X[2][3])
    return out


def rigid_product(A, B):
    A = [[float(v) for v in row] for row in A]
    B = [[float(v) for v in row] for row in B]
    out = np.empty((3, 4))
    for r in range(3):
        for c in range(4):
            out[r, c] = ((A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c]) + A[r][3] * (1.0 if c == 3 else 0.0)
    return out


def pair_transform(Tt, s, d):
    """X~ of the pair (s, d) at the poses Tt [N, 3, 4], float64 (not yet rounded)."""
    return rigid_product(Tt[d], rigid_inverse(Tt[s]))


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def _pivot_matrix(c):
    P = np.eye(6)
    P[:3, 3:] = -_skew(c)
    return P


def _adjoint(X):
    R, t = X[:, :3], X[:, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = R
    Ad[3:, 3:] = R
    Ad[3:, :3] = _skew(t) @ R
    return Ad


def _hessian(sums):
    H = np.zeros((6, 6))
    for col, (k, j) in enumerate(rr._TRI):
        H[k, j] = H[j, k] = sums[col]
    return H


# ---------------------------------------------------------------------------------------------------------------------
# one joint evaluation
# ---------------------------------------------------------------------------------------------------------------------
class JointEvaluation:
    """evs: {pair index: ref64_register.Evaluation} of the evaluated pairs; X: {pair index: X~ float64}; cost over them."""

    def __init__(self, evs, X, gate):
        self.evs, self.X, self.gate = evs, X, gate
        g2 = gate * gate
        num = sum(e.sums[27] + (e.candidates - e.valid) * g2 for e in evs.values())
        den = sum(e.candidates for e in evs.values())
        self.cost = num / den if den > 0 else g2
        self.ties = sum(e.ties for e in evs.values())
        self.tie_share = self.ties / max(den, 1)

    def cost_interval(self):
        """The interval the engine's joint cost may lie in: the pairs' intervals added."""
        g2 = self.gate * self.gate
        den = sum(e.candidates for e in self.evs.values())
        if den <= 0:
            return g2, g2
        lo = sum(e.lo[27] + (e.candidates - e.hi[28]) * g2 for e in self.evs.values()) / den
        hi = sum(e.hi[27] + (e.candidates - e.lo[28]) * g2 for e in self.evs.values()) / den
        return lo * (1 - 2 * rr.U), hi * (1 + 2 * rr.U)   # (the result is handed out as a float32)


def evaluate_pairs(maps, Tt, pairs, which, band, gate):
    evs, X = {}, {}
    for p in which:
        s, d = pairs[p]
        X[p] = pair_transform(Tt, s, d)
        evs[p] = rr.evaluate(maps[s], maps[d], X[p], band, gate)
    return JointEvaluation(evs, X, gate)


def joint_system(n_maps, pairs, active, anchor, je):
    """(H [6 (N - 1), 6 (N - 1)], g, pivots c [N, 3]) of the joint evaluation `je` over the active pairs."""
    c = np.zeros((n_maps, 3))
    for i in range(n_maps):
        acc, weight = np.zeros(3), 0.0
        for p in active:
            s, d = pairs[p]
            sums = je.evs[p].sums
            if d == i:
                acc += sums[29:32]
                weight += sums[28]
            elif s == i and sums[28] > 0:
                inv = rigid_inverse(je.X[p])
                acc += sums[28] * (inv[:, :3] @ (sums[29:32] / sums[28]) + inv[:, 3])
                weight += sums[28]
        if weight > 0:
            c[i] = acc / weight
    block = {i: (i if i < anchor else i - 1) for i in range(n_maps) if i != anchor}
    n = 6 * (n_maps - 1)
    H, g = np.zeros((n, n)), np.zeros(n)
    for p in active:
        s, d = pairs[p]
        sums = je.evs[p].sums
        Hp, gp = _hessian(sums), sums[21:27]
        J = {s: -_pivot_matrix(c[s]) @ _adjoint(je.X[p]).T, d: _pivot_matrix(c[d])}
        for a in (s, d):
            if a == anchor:
                continue
            ra = slice(6 * block[a], 6 * block[a] + 6)
            g[ra] += J[a] @ gp
            for b in (s, d):
                if b == anchor:
                    continue
                H[ra, slice(6 * block[b], 6 * block[b] + 6)] += J[a] @ Hp @ J[b].T
    return H, g, c


def _connected(n_maps, pairs, active, anchor):
    reached, todo = {anchor}, [anchor]
    while todo:
        m = todo.pop()
        for p in active:
            s, d = pairs[p]
            other = d if s == m else (s if d == m else None)
            if other is not None and other not in reached:
                reached.add(other)
                todo.append(other)
    return len(reached) == n_maps


def _solve(H, g, lam):
    d = np.diag(H)
    use = np.flatnonzero(d > 0)
    y = np.zeros(len(g))
    if len(use):
        y[use] = np.linalg.solve(H[np.ix_(use, use)] + lam * np.diag(d[use]), g[use])
    return y


def register_graph(maps, T0, pairs, anchor, **params):
    """dslam_register_graph on MapData.  T0: [N, 4, 4] in metres (entries taken as float32).  Returns (T [N, 4, 4] float32
    -- T0's own bytes if no step was accepted, and always for the anchor --, result dict as dslam_register_graph_result
    plus `pairs` (one dict per pair as dslam_register_pair_result), `trace` (one dict per evaluation: cost, tie_share, je,
    and for trial evaluations accepted, lam, margin and cost_slack as ref64_register.register records them) and `last`)."""
    pr = dict(DEFAULTS)
    pr.update({k: v for k, v in params.items() if v})
    pairs = [tuple(int(v) for v in p) for p in pairs]
    T0 = np.asarray(T0, np.float32)
    n_maps = len(maps)
    vs = maps[0].vs
    gate = float(np.float32(pr["residual_gate"]))
    Tt = np.stack([rr.voxel_transform(T0[i].astype(np.float64), vs) for i in range(n_maps)])

    first = evaluate_pairs(maps, Tt, pairs, range(len(pairs)), pr["band"], gate)
    active = [p for p in range(len(pairs)) if first.evs[p].valid >= pr["min_valid"]]
    good = JointEvaluation({p: first.evs[p] for p in active}, {p: first.X[p] for p in active}, gate)
    trace = [dict(cost=good.cost, tie_share=good.tie_share, je=good)]
    cost_first = good.cost
    evaluations, stop, accepted_any, lam = 1, -1, False, 1.0
    if not _connected(n_maps, pairs, active, anchor):
        stop = 3
    free = [i for i in range(n_maps) if i != anchor]
    while stop < 0:
        if evaluations >= pr["max_evaluations"]:
            stop = 1
            break
        H, g, c = joint_system(n_maps, pairs, active, anchor, good)
        y = _solve(H, g, lam).reshape(-1, 6)
        trial = Tt.copy()
        for k, i in enumerate(free):
            trial[i] = rr._increment(y[k], c[i], Tt[i])
        je = evaluate_pairs(maps, trial, pairs, active, pr["band"], gate)
        evaluations += 1
        accept = all(je.evs[p].valid >= pr["min_valid"] for p in active) and je.cost < good.cost
        (l1, h1), (l2, h2) = je.cost_interval(), good.cost_interval()
        trace.append(dict(cost=je.cost, tie_share=je.tie_share, je=je, accepted=accept, lam=lam,
                          margin=abs(je.cost - good.cost), cost_slack=(h1 - l1) + (h2 - l2)))
        if accept:
            used = lam
            Tt, good, accepted_any = trial, je, True
            lam = max(lam / 10.0, 1e-6)
            rot = max(np.linalg.norm(y[:, :3], axis=1))
            tr = max(np.linalg.norm(y[:, 3:], axis=1))
            if used <= 1.0 and rot < float(np.float32(pr["term_rotation"])) and tr < float(np.float32(pr["term_translation_voxels"])):
                stop = 0
        else:
            lam *= 10.0
            if lam > 1e6:
                stop = 2
    cond = 0.0 if stop == 3 else rr.conditioning(joint_system(n_maps, pairs, active, anchor, good)[0])
    T = T0.copy()
    if accepted_any:
        for i in free:
            T[i] = np.eye(4, dtype=np.float32)
            T[i, :3, :3] = Tt[i][:, :3].astype(np.float32)
            T[i, :3, 3] = (Tt[i][:, 3] * vs).astype(np.float32)
    per_pair = []
    for p in range(len(pairs)):
        e0 = first.evs[p]
        e1 = good.evs[p] if p in good.evs else e0
        per_pair.append(dict(candidates=e0.candidates, valid_first=e0.valid, valid_last=e1.valid, active=int(p in active),
                             cost_first=e0.cost, cost_last=e1.cost, last=e1))
    res = dict(evaluations=evaluations, stop_reason=stop, active_pairs=len(active), cost_first=cost_first,
               cost_last=good.cost, conditioning=cond, pairs=per_pair, trace=trace, last=good, first=first)
    return T, res
