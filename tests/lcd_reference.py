"""TEST INFRASTRUCTURE: a plain restatement of the loop-closure path of cl-slam_amd/csrc -- the non-GEMM ops of the
MobileNetV3-small encoder (lcd_ops.hip, as clslam_hip/lcd.py sequences them) and the retrieval kernels (search.hip) -- from
their formulas, not from the kernels' loops:

    stem              hardswish( scale * conv3x3 s2 p1 ((img - mean) / std) + shift ), 3 -> 16 channels, OIHW weights
    dwconv            act( scale * depthwise KxK (stride 1 | 2, pad K // 2) + shift ), weights [K*K][C]
    avgpool           mean over the pixels, per sample and channel
    se_gate           hardsigmoid( w2 relu( w1 pool + b1 ) + b2 )
    channel_scale     x * gate, the gate broadcast over the pixels
    hswish, hsigmoid  v * clamp(v + 3, 0, 6) / 6   and   clamp(v + 3, 0, 6) / 6   (common.h apply_act)
    l2_normalize      row * (1 / sqrt(<row, row>)) (faiss's fvec_renorm_L2); a row whose squared norm is not > 0 (zero, NaN) stays
    ip_scores         queries . db^T
    topk_desc         the k best (score, id) in descending score, equal scores by ascending id; a score that is NaN or not
                      above -FLT_MAX (-inf included) is never a match: it is not returned, and the places past the matches
                      hold -FLT_MAX / id -1 (faiss's heap starts at -FLT_MAX / -1 and admits only a greater score)
    diversity_commit  the three steps documented above diversity_commit_kernel, in float64 on numpy copies

Everything but diversity_commit is loop-free torch evaluated in `dtype`: float64 is the reference, float32 the yardstick ("what
the same formula loses in the kernel's own number format").  Activations are NHWC, weights in the library's layouts.  Nothing
here runs on the device."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_ELU, ACT_HSWISH, ACT_HSIGMOID = 0, 1, 2, 3, 4
FLT_MAX = float(np.finfo(np.float32).max)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def hswish(v):
    return v * torch.clamp(v + 3, 0, 6) / 6


def hsigmoid(v):
    return torch.clamp(v + 3, 0, 6) / 6


def act_fn(v, act):
    if act == ACT_RELU:
        return F.relu(v)
    if act == ACT_ELU:
        return F.elu(v)
    if act == ACT_HSWISH:
        return hswish(v)
    if act == ACT_HSIGMOID:
        return hsigmoid(v)
    return v


def _affine_act(y, scale, shift, act, dtype):
    """y NCHW -> act(scale * y + shift) NHWC"""
    y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    return act_fn(y, act).permute(0, 2, 3, 1).contiguous()


def stem(img, weight, scale, shift, dtype=F64):
    """img (B,3,H,W) un-normalised, weight (16,3,3,3) OIHW -> (B,Ho,Wo,16)"""
    x = (img.to(dtype) - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    return _affine_act(F.conv2d(x, weight.to(dtype), stride=2, padding=1), scale, shift, ACT_HSWISH, dtype)


def dwconv(x, weight, scale, shift, ksize, stride, act, dtype=F64):
    """x (B,H,W,C), weight (K*K, C) -> (B,Ho,Wo,C)"""
    C = x.shape[-1]
    w = weight.to(dtype).t().reshape(C, 1, ksize, ksize)
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w, stride=stride, padding=ksize // 2, groups=C)
    return _affine_act(y, scale, shift, act, dtype)


def avgpool(x, dtype=F64):
    """x (B,...,C) -> (B,C)"""
    return x.to(dtype).reshape(x.shape[0], -1, x.shape[-1]).mean(1)


def se_hidden(pool, w1, b1, dtype=F64):
    return F.relu(pool.to(dtype) @ w1.to(dtype).t() + b1.to(dtype))


def se_gate(pool, w1, b1, w2, b2, dtype=F64):
    """pool (B,C), w1 (S,C), b1 (S), w2 (C,S), b2 (C) -> (B,C)"""
    return hsigmoid(se_hidden(pool, w1, b1, dtype) @ w2.to(dtype).t() + b2.to(dtype))


def channel_scale(x, gate, dtype=F64):
    g = gate.to(dtype)
    return x.to(dtype) * g.view(g.shape[0], *([1] * (x.dim() - 2)), g.shape[1])


def l2_normalize(x, dtype=F64):
    x = x.to(dtype)
    n2 = (x * x).sum(1, keepdim=True)
    return torch.where(n2 > 0, x * (1 / n2.sqrt()), x)


def ip_scores(db, q, dtype=F64):
    """db (n,d), q (nq,d) -> (nq,n)"""
    return q.to(dtype) @ db.to(dtype).t()


def topk_desc(scores, k):
    """scores (nq,n) of any float dtype -> values (nq,k) in that dtype, ids (nq,k) int64"""
    s = scores.clone()
    nq, n = s.shape
    match = s > -FLT_MAX                                   # False for NaN, -inf and -FLT_MAX itself
    key = torch.where(match, s, torch.full_like(s, -float('inf')))
    order = torch.sort(key, dim=1, descending=True, stable=True)[1]     # stable: equal scores keep ascending position
    val = torch.full((nq, k), -FLT_MAX, dtype=s.dtype)
    idx = torch.full((nq, k), -1, dtype=torch.int64)
    m = min(k, n)
    if m:
        o = order[:, :m]
        ok = torch.gather(match, 1, o)
        val[:, :m] = torch.where(ok, torch.gather(s, 1, o), val[:, :m])
        idx[:, :m] = torch.where(ok, o, idx[:, :m])
    return val, idx


def diversity_commit(db, S, occupied, nslots, max_slots, capacity, threshold, q, scores=None):
    """One candidate, IN PLACE on the float64 numpy arrays db (max_slots,d), S (ld,ld) and the bool / uint8 vector occupied.
    scores: <db[j], q> per slot as the caller computed them (default: in float64 from db).
    -> dict(accepted, slot, evict, count, similarity, margin_accept, margin_evict, colsum_terms): the margins are the
    distances of the two decisions from their alternatives (threshold - similarity; best - second best eviction score),
    colsum_terms the sum of |term| of the winning eviction score."""
    q = np.asarray(q, dtype=np.float64)
    sc = db[:nslots] @ q if scores is None else np.asarray(scores, dtype=np.float64)[:nslots]
    occ = np.asarray(occupied[:nslots], dtype=bool)
    similarity = float(sc[occ].max()) if occ.any() else 0.0           # numpy's max / argmax: the first maximum
    free = np.nonzero(~occ)[0]
    slot = int(free[0]) if len(free) else nslots
    count = int(occ.sum())
    out = dict(accepted=0, slot=-1, evict=-1, count=count, similarity=similarity, margin_accept=abs(threshold - similarity),
               margin_evict=np.inf, colsum_terms=0.0, nearest=int(np.nonzero(occ)[0][np.argmax(sc[occ])]) if occ.any() else -1)
    if not (similarity < threshold and slot < max_slots):
        return out
    db[slot] = q
    n_after = max(nslots, slot + 1)
    row = np.full(n_after, -1.0)
    row[:nslots][occ] = sc[occ]
    row[slot] = float(q @ q)
    S[slot, :n_after] = row
    S[:n_after, slot] = row
    occupied[slot] = 1
    count += 1
    evict = -1
    if count > capacity:
        o = np.nonzero(np.asarray(occupied[:n_after], dtype=bool))[0]
        sub = S[np.ix_(o, o)]
        col = sub.sum(0) - np.diag(sub)
        j = int(np.argmax(col))                                      # first maximum
        evict = int(o[j])
        rest = np.delete(col, j)
        out['margin_evict'] = float(col[j] - rest.max()) if len(rest) else np.inf
        out['colsum_terms'] = float(np.abs(sub).sum(0).max())
        S[evict, :n_after] = -1.0
        S[:n_after, evict] = -1.0
        occupied[evict] = 0
        count -= 1
    out.update(accepted=1, slot=slot, evict=evict, count=count)
    return out
