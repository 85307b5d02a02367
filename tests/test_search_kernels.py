"""The retrieval kernels of csrc/search.hip one C entry point at a time (clslam_l2_normalize_rows, clslam_ip_scores,
clslam_topk_desc, clslam_diversity_commit), on buffers pre-filled with NaN, against the restatement of tests/lcd_reference.py.
Conventions as documented at the top of tests/test_conv_layers.py and tests/test_loss_kernels.py.

Bounds.
  * l2_normalize, ip_scores: largest absolute error and relative L2 per row against float64, at most 4 x the figure of the same
    restatement in torch float32 (formed first; median-row fallback).  Both kernels treat every row on its own, so the measured
    comparison runs once per d on the largest case (n = 5: two workgroups, a ragged last one; nq = 3) and every smaller
    (n, nq) must reproduce its rows BITWISE while the rows past n stay NaN.  On top, every dot product is held to the textbook
    |error| <= chain * 2^-24 * sum |term| (chain = fma's of a lane + the 6 levels of the wave reduction) and every norm to
    | ||row|| - 1 | <= (chain + 4) * 2^-24 (the sum, its square root, the reciprocal, the product, the norm of rounded numbers).
  * topk_desc sorts given fp32 numbers and does no arithmetic: ids and values equal the restatement exactly, on hand-built
    and on random input (scores drawn from few distinct values, so that ties are everywhere, chunk boundary included).
    ip_scores -> topk_desc chained is compared with the float64 ranking: an id may differ only where the float64 scores of the
    two ids differ by less than the dot-product bound; such places are capped at 1 % (none occur with the seeds used).
  * -inf (settled in the header of search.hip): like NaN never a match, returned as padding (-FLT_MAX, -1) -- what faiss's
    heap, which starts at -FLT_MAX and admits only a greater score, returns.  Before the fix the kernel kept the id of a
    -inf score but sorted it BEHIND the padding: test_topk_hand_built[specials-*] saw [.., -1, -1, id].
  * diversity_commit: the 40-candidate sequence and the 300-slot sequence use components that are multiples of 1/8, so every
    product, dot product and column sum is exact in fp32: db, S, occupied, result[0..4] and the similarity equal the float64
    restatement EXACTLY after every call, ties included, nothing excused.  The sequence of random unit vectors compares S and
    the similarity under the dot-product bound (chain = 1 + 6, q.q: 1 + 8 levels of the block tree), the column sums enter
    only through the eviction decision: the seed is chosen so that every accept / evict margin of the float64 restatement is
    above the fp32 resolution (asserted first, on the CPU), and then every decision must equal the float64 one.

Measured figures (kernel | torch fp32, against float64), the worst case of each quantity; emu = kernel sources on the CPU
emulator, hip = gfx950 (printed per case with -s):
  quantity                              emu kernel | fp32   (ratio)        hip kernel | fp32   (ratio)
  l2_normalize max                        5.24e-08 |  4.22e-08 (1.24x)       5.96e-08 |  5.96e-08 (1.00x)
  l2_normalize channel rel L2             7.13e-08 |  6.30e-08 (1.13x)       5.96e-08 |  5.96e-08 (1.00x)
  l2_normalize | norm - 1 | / derived bound 0.118                              0.129
  ip_scores max                           3.21e-07 |  2.00e-07 (1.61x)       3.21e-07 |  2.00e-07 (1.61x)
  ip_scores channel rel L2                2.07e-07 |  1.61e-07 (1.28x)       6.88e-08 |  7.62e-08 (0.90x)
  ip_scores dot error / derived bound    0.167                              0.157

One-line mutations of search.hip (CPU emulator, scratch copies) and the test that fails; "before" = whether
tests/test_flat_index.py and tests/test_replay_lcd.py as they stood caught it on the emulator:
  before() `a > b || (a == b && ia < ib)` -> `a > b` (the tie-break of topk_sort_kernel)
                     test_topk_random_with_ties (14 cases), test_topk_hand_built (8), test_diversity_commit_sequence  before: yes
                     (test_flat_index.py::test_reference_usage_patterns, its five duplicates)
  ip_scores_kernel scalar loop `i = lane` -> `i = lane + 1`
                     test_ip_scores[10], [63], test_ip_scores_then_topk_against_the_float64_ranking     before: yes
                     (test_search_matches_restatement[300-10-100-2], the one d % 4 != 0 case)
  diversity_commit_kernel `acc > bv` -> `acc >= bv`
                     test_diversity_commit_more_than_256_slots (slot 261 evicted instead of 5)           before: no
  topk_sort_kernel as it was before this change (-inf keeps its id and sorts behind the padding)
                     test_topk_hand_built[specials-10-10], [specials-8192-2048]                          before: no
"""
import numpy as np
import pytest
import torch

import lcd_reference as L
from clslam_hip import _lib, ops
from emu_util import BACKENDS, use_backend
from test_conv_layers import ROWS, U, _chain_bound, _flush, _measured

F32, F64 = torch.float32, torch.float64
NAN, INF = float('nan'), float('inf')
FLT_MAX = L.FLT_MAX


def _decades(g, n):
    e = torch.rand(n, generator=g) * 2 - 1
    if n > 1:
        e[0], e[n - 1] = -1.0, 1.0
    return (10.0 ** e)[torch.randperm(n, generator=g)]


def _call(name, *args):
    _lib.get_lib().call(name, *args)


# ---- l2_normalize ---------------------------------------------------------------------------------------------------------------
L2_D = [1, 3, 63, 64, 65, 576]


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('d', L2_D)
def test_l2_normalize_rows(backend, d, capsys):
    """n = 5 measured (row 1 is a zero row and stays zero), n in {1, 3, 4} bitwise the same rows with the rest untouched"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(100 + d)
    x = torch.randn(5, d, generator=g) * _decades(g, d) * _decades(g, 5).view(5, 1)
    x[1] = 0.0
    ref64, ref32 = L.l2_normalize(x, F64), L.l2_normalize(x, F32)
    full = None
    for n in (5, 1, 3, 4):
        buf = torch.full((5, d), NAN)
        buf[:n] = x[:n]
        buf = buf.to(dev)
        _call('clslam_l2_normalize_rows', buf.data_ptr(), n, d, ops._stream(buf))
        got = buf.cpu()
        assert torch.isnan(got[n:]).all(), ('rows past n were touched', n)
        if n == 5:
            full = got
            assert torch.equal(got[1], torch.zeros(d)), 'a zero row must stay zero'
            _measured(backend, f'l2_normalize d={d}', 'rows', got.t(), ref64.t(), ref32.t())
            norm = got.double().norm(dim=1)
            chain = -(-d // 64) + 6
            keep = torch.tensor([0, 2, 3, 4])
            dev1 = (norm[keep] - 1).abs().max()
            ROWS.append(f'  [{backend}] l2_normalize d={d:<4} | norm - 1 | / bound {float(dev1) / ((chain + 4) * U):6.3f}')
            assert float(dev1) <= (chain + 4) * U, (d, float(dev1))
        else:
            assert torch.equal(got[:n], full[:n]), ('a row depends on how many rows the launch has', n)
    _flush(capsys)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('d', [3, 65])
def test_l2_normalize_non_finite_rows_stay_alone(backend, d):
    """five rows = two workgroups, four waves in the first: a row with a NaN (left as it is: its norm is not > 0) and a row
    with an inf (finite entries -> 0, the inf -> NaN, as x / sqrt(inf) gives) do not disturb the rows next to them"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(7 + d)
    x = torch.randn(5, d, generator=g)
    x[1, d // 2], x[2, d - 1] = NAN, INF
    ref = L.l2_normalize(x, F32)
    buf = x.clone().to(dev)
    _call('clslam_l2_normalize_rows', buf.data_ptr(), 5, d, ops._stream(buf))
    got = buf.cpu()
    clean = torch.tensor([0, 3, 4])
    full = L.l2_normalize(x[clean], F64)
    assert float((got[clean].double() - full).abs().max()) <= (-(-d // 64) + 10) * U
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(got[1].nan_to_num(7.0), x[1].nan_to_num(7.0)), 'the NaN row is left as it is'
    assert torch.equal(got[2][:-1], torch.zeros(d - 1)) and torch.isnan(got[2, -1])


# ---- ip_scores ------------------------------------------------------------------------------------------------------------------
IP_D = [4, 10, 63, 252, 256, 260, 576]


def _ip_chain(d):
    return (4 * -(-d // 256) if d % 4 == 0 else -(-d // 64)) + 6


def _run_ip(dev, db, q, n, nq):
    out = torch.full((3, 5), NAN, device=dev)
    dbd, qd = db[:n].contiguous().to(dev), q[:nq].contiguous().to(dev)
    _call('clslam_ip_scores', dbd.data_ptr(), qd.data_ptr(), out.data_ptr(), n, db.shape[1], nq, ops._stream(out))
    flat = out.cpu().reshape(-1)
    assert torch.isnan(flat[nq * n:]).all(), ('scores past nq * n were touched', n, nq)
    return flat[:nq * n].reshape(nq, n)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('d', IP_D)
def test_ip_scores(backend, d, capsys):
    """d % 4 == 0: the 16-byte path (d = 252: a ragged last stride; 260: a second stride of one lane); otherwise the scalar
    path (d = 10, 63: lanes without an element).  n = 5, nq = 3 measured, n in {1, 4} x nq in {1, 3} bitwise its sub-blocks."""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(200 + d)
    gain = _decades(g, d)
    db = (torch.randn(5, d, generator=g) * gain).contiguous()
    q = (torch.randn(3, d, generator=g) / gain).contiguous()           # products of unit size, no channel drowned
    ref64, ref32 = L.ip_scores(db, q, F64), L.ip_scores(db, q, F32)
    abs64 = L.ip_scores(db.abs(), q.abs(), F64)
    full = _run_ip(dev, db, q, 5, 3)
    _measured(backend, f'ip_scores d={d}', 'scores', full, ref64, ref32)
    _chain_bound(backend, f'ip_scores d={d}', 'scores', full, ref64, abs64, _ip_chain(d))
    for n in (1, 4, 5):
        for nq in (1, 3):
            assert torch.equal(_run_ip(dev, db, q, n, nq), full[:nq, :n]), ('a score depends on the launch size', n, nq)
    _flush(capsys)


# ---- topk_desc ------------------------------------------------------------------------------------------------------------------
def _run_topk(dev, scores, k):
    """scores (nq, n) fp32 -> (values (nq,k), ids (nq,k)) as clslam_topk_desc writes them"""
    nq, n = scores.shape
    chunks = _lib.get_lib().cdll.clslam_topk_chunks(n)
    sd = scores.contiguous().to(dev)
    val = torch.full((nq, k), NAN, device=dev)
    idx = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    cv = torch.full((nq, chunks, k), NAN, device=dev) if chunks > 1 else None
    ci = torch.full((nq, chunks, k), -7, dtype=torch.int32, device=dev) if chunks > 1 else None
    _call('clslam_topk_desc', sd.data_ptr() if n else None, n, nq, k, None if cv is None else cv.data_ptr(),
          None if ci is None else ci.data_ptr(), val.data_ptr(), idx.data_ptr(), ops._stream(val))
    return val.cpu(), idx.cpu().long()


def _assert_topk_exact(scores, k, val, idx, what):
    rv, ri = L.topk_desc(scores, k)
    assert torch.equal(idx, ri), (what, 'ids', idx[0, :12].tolist(), ri[0, :12].tolist(),
                                  (idx != ri).nonzero()[:4].tolist())
    assert torch.equal(val, rv), (what, 'values')
    pad = idx == -1
    assert bool((val[pad] == -FLT_MAX).all())
    assert bool((pad[:, 1:] >= pad[:, :-1]).all()), (what, 'a real id after a padding id')


def _topk_sizes():
    out = []
    for n in (0, 1, 4095, 4096, 4097, 8192):
        chunks = max(1, -(-n // 4096))
        for k in (1, 100, 2048, 4096):
            if chunks * k <= 4096:
                out.append((n, k))
    return out


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('n,k', _topk_sizes())
def test_topk_random_with_ties(backend, n, k):
    """two queries; scores drawn from 97 distinct values (n >= 4095: every value many times, ties across the chunk boundary)
    for the first, distinct values for the second; k > n (n = 0, 1) pads; k = 2048 at two chunks and 4096 at one are the
    chunks * k <= 4096 limit"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(1000 + n + k)
    s = torch.empty(2, n)
    if n:
        s[0] = torch.randint(-48, 49, (n,), generator=g).float() / 16
        s[1] = torch.randn(n, generator=g)
    val, idx = _run_topk(dev, s, k)
    _assert_topk_exact(s, k, val, idx, (n, k))


def _hand_built():
    cases = {}
    for n, k in ((4097, 100), (8192, 2048), (4096, 4096), (5, 9)):
        cases[f'all-equal-{n}-{k}'] = (torch.full((1, n), 0.25), k)
    g = torch.Generator().manual_seed(5)
    for n, k in ((4097, 100), (8192, 100), (8192, 2048)):
        s = -torch.rand(1, n, generator=g) - 1                       # distinct, all below the runs
        s[0, 4090:min(n, 4102)] = 1.0                                # the best: a run over elements 4095 | 4096
        s[0, 100:104] = 1.0                                          # ... that continues a run of the first chunk
        if n > 4200:
            s[0, 4094:4098] = 1.0
            s[0, 4000:4090] = 0.5                                    # second best: ends right at the run
            s[0, 4102:4200] = 0.5                                    # ... and goes on behind it
        cases[f'runs-{n}-{k}'] = (s, k)
    s = torch.tensor([[0.5, NAN, INF, -INF, 0.5, -1.0, -FLT_MAX, INF, 2.0, NAN]])
    cases['specials-10-10'] = (s, 10)
    cases['specials-10-3'] = (s, 3)
    s = torch.randn(1, 4097, generator=g)
    s[0, 4096] = -INF                                                # the second chunk holds nothing but a -inf
    s[0, 17], s[0, 4095], s[0, 0] = NAN, INF, -INF
    cases['specials-4097-100'] = (s, 100)
    cases['specials-4097-2048'] = (s.clone(), 2048)
    s = torch.full((1, 8192), -INF)
    s[0, 8000], s[0, 4096], s[0, 5] = 1.0, NAN, 1.0
    cases['specials-8192-2048'] = (s, 2048)
    return cases


HAND = _hand_built()


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', list(HAND))
def test_topk_hand_built(backend, name):
    """exact, nothing excused: equal scores in ascending id (inside a chunk and through the merge of the chunk winners), +inf
    first, NaN / -inf / -FLT_MAX never returned, no real id behind a padding id"""
    dev = use_backend(backend)
    s, k = HAND[name]
    val, idx = _run_topk(dev, s, k)
    _assert_topk_exact(s, k, val, idx, name)
    if name == 'specials-10-10':
        assert idx[0].tolist() == [2, 7, 8, 0, 4, 5, -1, -1, -1, -1]
    if name.startswith('all-equal'):
        n = s.shape[1]
        assert idx[0].tolist() == list(range(min(n, k))) + [-1] * (k - min(n, k))


@pytest.mark.parametrize('backend', BACKENDS)
def test_ip_scores_then_topk_against_the_float64_ranking(backend):
    """n = 4097, d = 10 (scalar path, two chunks), k = 100: where the kernel's id differs from the float64 ranking the two
    float64 scores differ by less than the dot-product bound; at most 1 % of the places (the fp32 restatement is held to the
    same first)"""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(31)
    n, d, nq, k = 4097, 10, 2, 100
    db = L.l2_normalize(torch.randn(n, d, generator=g), F32).float()
    q = L.l2_normalize(torch.randn(nq, d, generator=g), F32).float()
    s64 = L.ip_scores(db, q, F64)
    _, i64 = L.topk_desc(s64, k)
    res = 2 * _ip_chain(d) * U * L.ip_scores(db.abs(), q.abs(), F64).max()

    def excused(ids, who):
        bad = ids != i64
        gap = (torch.gather(s64, 1, ids.clamp_min(0)) - torch.gather(s64, 1, i64)).abs()
        assert bool((gap[bad] <= res).all()), (who, 'ranking differs with a margin above the fp32 resolution', float(gap[bad].max()))
        assert int(bad.sum()) <= 0.01 * bad.numel(), (who, int(bad.sum()))
        return int(bad.sum())

    excused(L.topk_desc(L.ip_scores(db, q, F32), k)[1], 'fp32 restatement')
    sc = torch.full((nq, n), NAN, device=dev)
    dbd, qd = db.to(dev), q.to(dev)
    _call('clslam_ip_scores', dbd.data_ptr(), qd.data_ptr(), sc.data_ptr(), n, d, nq, ops._stream(sc))
    val, idx = _run_topk(dev, sc.cpu(), k)
    excused(idx, 'kernel')
    assert float((val.double() - torch.gather(s64, 1, idx)).abs().max()) <= res


# ---- diversity_commit -----------------------------------------------------------------------------------------------------------
class _Buffer:
    """the device state of one diversity buffer (db NaN-filled: a free slot's row is never to be used) and its float64 twin"""

    def __init__(self, dev, d, capacity, max_slots, ld):
        self.dev, self.d, self.capacity, self.max_slots, self.ld = dev, d, capacity, max_slots, ld
        self.db = torch.full((max_slots, d), NAN, device=dev)
        self.S = torch.full((ld, ld), -1.0, device=dev)
        self.occ = torch.zeros(max_slots, dtype=torch.uint8, device=dev)
        self.scores = torch.full((max_slots,), NAN, device=dev)
        self.result = torch.full((5,), -7, dtype=torch.int32, device=dev)
        self.sim = torch.full((1,), NAN, device=dev)
        self.nslots = 0
        self.rdb = np.full((max_slots, d), np.nan)
        self.rS = np.full((ld, ld), -1.0)
        self.rocc = np.zeros(max_slots, dtype=np.uint8)

    def add(self, q, threshold):
        """-> (kernel result[0..3], kernel similarity, restatement dict)"""
        qd = torch.tensor(q, dtype=F32).to(self.dev)
        stream = ops._stream(qd)
        if self.nslots:
            _call('clslam_ip_scores', self.db.data_ptr(), qd.data_ptr(), self.scores.data_ptr(), self.nslots, self.d, 1, stream)
        self.result.fill_(-7)
        self.sim.fill_(NAN)
        _call('clslam_diversity_commit', self.db.data_ptr(), self.S.data_ptr(), self.ld, self.occ.data_ptr(), self.nslots,
              self.max_slots, self.d, self.capacity, float(threshold), qd.data_ptr(), self.scores.data_ptr(),
              self.result.data_ptr(), self.sim.data_ptr(), stream)
        res = self.result.cpu()
        sim = float(self.sim.cpu())
        assert float(res[4:5].view(F32)) == sim, 'result[4] holds the bits of the similarity'
        ref = L.diversity_commit(self.rdb, self.rS, self.rocc, self.nslots, self.max_slots, self.capacity,
                                 float(np.float32(threshold)), np.asarray(q, dtype=np.float32).astype(np.float64))
        if ref['accepted']:
            self.nslots = max(self.nslots, ref['slot'] + 1)
        return [int(v) for v in res[:4]], sim, ref

    def assert_state(self, step, res, sim, ref, exact=True):
        want = [ref['accepted'], ref['slot'], ref['evict'], ref['count']]
        assert res == want, (step, 'result', res, want, ref['margin_accept'], ref['margin_evict'])
        assert np.array_equal(self.occ.cpu().numpy(), self.rocc), (step, 'occupied')
        assert np.array_equal(self.db.cpu().numpy().astype(np.float64), self.rdb, equal_nan=True), (step, 'db')
        S = self.S.cpu().numpy().astype(np.float64)
        assert np.array_equal(S == -1.0, self.rS == -1.0), (step, 'the -1 marks of S')
        if exact:
            assert sim == ref['similarity'], (step, 'similarity', sim, ref['similarity'])
            assert np.array_equal(S, self.rS), (step, 'S', np.argwhere(S != self.rS)[:4].tolist())
        else:
            n = self.nslots
            rows = np.nan_to_num(np.abs(self.rdb[:n]))
            norm1 = rows @ rows.T                                   # sum |term| of every stored dot product
            bound = np.full_like(self.rS, 0.0)
            bound[:n, :n] = 9 * U * norm1
            assert bool((np.abs(S - self.rS) <= bound).all()), (step, 'S', float(np.abs(S - self.rS).max()))
            assert abs(sim - ref['similarity']) <= 7 * U * float(norm1.max()), (step, 'similarity')


def _grid(g, n, d, lo=-8, hi=8):
    return (torch.randint(lo, hi + 1, (n, d), generator=g).double() / 8).numpy()


@pytest.mark.parametrize('backend', BACKENDS)
def test_diversity_commit_sequence(backend):
    """40 candidates, d = 12, capacity = 6, max_slots = 8, ld = 8, components multiples of 1/8 (everything exact in fp32):
    an exact duplicate (ties the nearest argmax, and later the eviction argmax: its two copies have equal column sums, the
    first one goes), a threshold equal to the similarity (rejected, `<` is strict; accepted one ulp above), and at the end a
    candidate that would be accepted but finds every one of the 8 slots taken (slot == max_slots: rejected)."""
    dev = use_backend(backend)
    buf = _Buffer(dev, 12, 6, 8, 8)
    g = torch.Generator().manual_seed(3)
    cand = _grid(g, 40, 12)
    big = np.full(12, 1.0)                                  # most similar to everything with positive sums: evicted first
    cand[3] = big
    cand[4] = big                                           # exact duplicate: accepted only under a threshold above q.q
    cand[5:9] = np.abs(cand[5:9])                           # four samples in the positive orthant: the duplicates lead the sums
    seen = dict(reject=0, accept=0, evict=0, tie_evict=0, strict=0)
    for i, q in enumerate(cand):
        thr = 100.0 if i < 12 else 1.5
        if i in (20, 30):                                   # threshold == similarity: rejected; the same candidate one ulp up
            probe = L.diversity_commit(buf.rdb.copy(), buf.rS.copy(), buf.rocc.copy(), buf.nslots, 8, 6, 1e9, q)
            thr = probe['similarity']
            assert np.float32(thr) == thr
            res, sim, ref = buf.add(q, thr)
            buf.assert_state((i, 'strict'), res, sim, ref)
            assert res[0] == 0 and sim == thr
            seen['strict'] += 1
            thr = float(np.nextafter(np.float32(thr), np.float32(np.inf)))
        res, sim, ref = buf.add(q, thr)
        buf.assert_state(i, res, sim, ref)
        seen['accept' if res[0] else 'reject'] += 1
        seen['evict'] += res[2] >= 0
        seen['tie_evict'] += ref['margin_evict'] == 0.0
    assert seen['strict'] == 2 and seen['reject'] >= 5 and seen['evict'] >= 10 and seen['tie_evict'] >= 1, seen
    # every slot taken: the state a caller with capacity = max_slots reaches
    buf.occ.fill_(1)
    buf.rocc[:] = 1
    buf.nslots = 8
    filler = torch.tensor(_grid(g, 8, 12), dtype=F32)
    buf.db.copy_(filler.to(dev))
    buf.rdb[:] = filler.double().numpy()
    res, sim, ref = buf.add(-big, 1e9)
    buf.assert_state('full', res, sim, ref)
    assert res == [0, -1, -1, 8]


@pytest.mark.parametrize('backend', BACKENDS)
def test_diversity_commit_more_than_256_slots(backend):
    """d = 8, capacity = 299, 304 slots: every strided loop of the kernel takes a second trip.  Slots 5 and 261 (one thread
    handles both) hold the same vector, the one most similar to all others: the 300th sample evicts slot 5, the FIRST maximum,
    and the next one, which re-uses slot 5, evicts 261.  Components are multiples of 1/8: exact, nothing excused."""
    dev = use_backend(backend)
    buf = _Buffer(dev, 8, 299, 304, 304)
    g = torch.Generator().manual_seed(11)
    cand = _grid(g, 306, 8, 0, 7)
    cand[5] = cand[261] = 1.0
    evicted = []
    for i, q in enumerate(cand):
        res, sim, ref = buf.add(q, 1e9 if i != 303 else 0.5)          # candidate 303 is rejected (similarity >= 0.5)
        if i >= 295 or i in (0, 1, 6, 255, 256, 257, 262):
            buf.assert_state(i, res, sim, ref)
        else:
            assert res == [ref['accepted'], ref['slot'], ref['evict'], ref['count']] and sim == ref['similarity'], i
        if res[2] >= 0:
            evicted.append(res[2])
    assert evicted[:2] == [5, 261] and len(evicted) == 6, evicted
    assert buf.nslots == 300


@pytest.mark.parametrize('backend', BACKENDS)
def test_diversity_commit_unit_vectors(backend):
    """40 random unit vectors (what the replay buffer stores), d = 12, capacity = 6: S and the similarity under the dot-product
    bound, every decision equal to the float64 one -- the seed keeps every float64 margin above the fp32 resolution of the
    quantity compared (asserted here first: 7 * 2^-24 * sum |term| for the accept test, (slots + 9) * 2^-24 * sum |term| for the
    column sums), so nothing is excused."""
    dev = use_backend(backend)
    g = torch.Generator().manual_seed(8)
    base = torch.randn(4, 12, generator=g)
    cand = base[torch.randint(0, 4, (40,), generator=g)] + 0.45 * torch.randn(40, 12, generator=g)   # four loose clusters
    cand = L.l2_normalize(cand, F32).float().numpy()
    thr = 0.8
    twin = _Buffer(torch.device('cpu'), 12, 6, 8, 8)                 # float64 state only: the margins of the sequence
    ns, steps = 0, []
    for q in cand:
        r = L.diversity_commit(twin.rdb, twin.rS, twin.rocc, ns, 8, 6, float(np.float32(thr)), q.astype(np.float64))
        ns = max(ns, r['slot'] + 1) if r['accepted'] else ns
        assert r['margin_accept'] > 4 * 7 * U, ('pick another seed: accept margin', r['margin_accept'])
        assert r['margin_evict'] > 4 * (8 + 9) * U * max(r['colsum_terms'], 1.0), ('pick another seed: evict margin', r['margin_evict'])
        steps.append(r)
    assert sum(r['accepted'] for r in steps) >= 10 and sum(r['evict'] >= 0 for r in steps) >= 4
    assert sum(not r['accepted'] for r in steps) >= 10
    buf = _Buffer(dev, 12, 6, 8, 8)
    for i, q in enumerate(cand):
        res, sim, ref = buf.add(q, thr)
        buf.assert_state(i, res, sim, ref, exact=False)
