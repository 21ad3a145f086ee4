"""reduce.quantile / nanquantile on the GPU against the exact model of tests/_quantile_ref.py.

Shapes: the smallest that reach every branch of the three kernel forms (rows of <= 32 elements at 8 / 16 / 32
lanes per row, rows in registers up to 1024, multi-rank radix selection over HBM beyond), with a ragged last
workgroup, a base pointer one element off a 16-byte line, and one row spread over 65 chunks.

Bounds: 'lower' / 'higher' / 'nearest' return an element: bit for bit.  'linear' / 'midpoint' are held to
4 eps_T max(|v_lo|, |v_hi|) of the exact value: the kernel rounds three times in float64 (b - a, the product,
the sum), each by at most eps64 max(|v_lo|, |v_hi|), and once to T -- under eps_T for float32, under 3 eps_T for
float64.  That last step presupposes a result in T's normal range, so the data plants denormals one value per row
and in rows without zeros: every pair of unequal neighbours then holds a normal number (the order-statistic
modes check the denormals themselves, bit for bit).
Worst ratio observed on MI355X: profiles/quantile_accuracy.md.
"""
import numpy as np
import pytest
import torch
import _quantile_ref as QR

pytestmark = pytest.mark.gpu

QLIST = [0.0, 1.0, 0.5, 0.25, 1 / 3, 0.999, 1e-9]
DT = {'f32': (torch.float32, np.float32, 2.0 ** -23), 'f64': (torch.float64, np.float64, 2.0 ** -52)}
KINDS = ('ints', 'normal', 'sorted', 'reversed', 'constant', 'zeros_infs', 'denormal_pos', 'denormal_neg',
         'nan_one', 'nan_all_but_one', 'nan_all')


@pytest.fixture(scope='module')
def R():
    from nitorch_fastmath_amd import reduce
    return reduce


def make_row(kind, red, npdt, rng):
    normal = (rng.standard_normal(red) * 2.0 ** int(rng.integers(-20, 21))).astype(npdt)   # a power of two per row
    normal[normal == 0] = 1
    ints = rng.integers(-3, 4, red).astype(npdt)                                            # heavy ties
    where = rng.permutation(red)
    if kind == 'ints':
        return ints
    if kind == 'normal':
        return normal
    if kind == 'sorted':
        return np.sort(normal)
    if kind == 'reversed':
        return np.sort(normal)[::-1].copy()
    if kind == 'constant':
        return np.full(red, normal[0], dtype=npdt)
    if kind == 'zeros_infs':
        plant = np.array([0.0, -0.0, np.inf, -np.inf, np.inf, -np.inf], dtype=npdt)
        ints[where[:6]] = plant[:min(6, red)]
        return ints
    if kind in ('denormal_pos', 'denormal_neg'):
        d = npdt(np.finfo(npdt).smallest_subnormal * 37) * (1 if kind == 'denormal_pos' else -1)
        normal[where[:2]] = d
        return normal
    if kind == 'nan_one':
        normal[where[0]] = np.nan
        return normal
    if kind == 'nan_all_but_one':
        keep = normal[where[0]]
        normal[:] = np.nan
        normal[where[0]] = keep
        return normal
    assert kind == 'nan_all'
    return np.full(red, np.nan, dtype=npdt)


def tensors(rows, red, npdt, seed, kinds=KINDS):
    """(rows, red) arrays that together hold every kind of row"""
    rng = np.random.default_rng(seed)
    out = []
    for base in range(0, len(kinds), rows):
        out.append(np.stack([make_row(kinds[(base + r) % len(kinds)], red, npdt, rng) for r in range(rows)]))
    return out


def same_bits(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def on_gpu(x, dev, offset):
    """the array on the GPU, contiguous; offset: at a base pointer one element off (the flat buffer from 1 on)"""
    if not offset:
        return torch.from_numpy(x).to(dev)
    flat = torch.empty(x.size + 1, dtype=torch.from_numpy(x).dtype, device=dev)
    t = flat[1:].view(x.shape)
    t.copy_(torch.from_numpy(x))
    assert t.is_contiguous() and t.data_ptr() % 16 != 0
    return t


def check(R, x, dev, dn, omitnan, offset=False):
    tdt, npdt, eps = DT[dn]
    t = on_gpu(x, dev, offset)
    before = t.clone()
    model = QR.quantiles(x, QLIST, omitnan)
    got = {}
    for interp in QR.INTERPS:
        g = R.quantile(t, QLIST, dim=1, omitnan=omitnan, inplace=True, interpolation=interp)
        assert g.shape == (len(QLIST), x.shape[0]) and g.dtype == tdt
        got[interp] = g.cpu().numpy()
        exact, vlo, vhi = model[interp]
        if interp in ('lower', 'higher', 'nearest'):
            want = QR.as_dtype(exact, npdt)
            assert np.array_equal(got[interp], want, equal_nan=True), (interp, x.shape, got[interp], want)
        else:
            ratio = QR.worst_ratio(got[interp], exact, vlo, vhi, eps)
            print(f'QACC {dn} {interp} red={x.shape[1]} rows={x.shape[0]} omitnan={int(omitnan)} ratio={ratio:.4f}')
            assert ratio <= 4.0, (interp, x.shape, ratio)
    # a scalar q: the reduced shape, the same bits
    fn = R.nanquantile if omitnan else R.quantile
    one = fn(t, QLIST[3], dim=1)
    assert one.shape == (x.shape[0],) and same_bits(one.cpu().numpy(), got['linear'][3])
    # the median is the lower quantile at 0.5: ties every form to the kernels of `median`
    med = R.median(t, dim=1, omitnan=omitnan).cpu().numpy()
    assert same_bits(fn(t, 0.5, dim=1, interpolation='lower').cpu().numpy(), med)
    assert same_bits(got['lower'][2], med)
    assert torch.equal(t.view(torch.int32 if dn == 'f32' else torch.int64),
                       before.view(torch.int32 if dn == 'f32' else torch.int64))   # the input is never written


FORM1 = [(rows, red) for red in (1, 2, 3, 8, 9, 17, 32) for rows in (1, 67)]
FORM2 = [(rows, red) for red in (33, 64, 65, 257, 1000, 1024) for rows in (1, 9)]
FORM3 = [(rows, red) for red in (1025, 16385, 40000) for rows in (1, 3)]


@pytest.mark.parametrize('omitnan', [False, True])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('rows,red', FORM1 + FORM2)
def test_rows_in_registers(R, dev, rows, red, dn, omitnan):
    for x in tensors(rows, red, DT[dn][1], 1000 * red + rows):
        check(R, x, dev, dn, omitnan)


@pytest.mark.parametrize('omitnan', [False, True])
@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('offset', [False, True])
@pytest.mark.parametrize('rows,red', FORM3)
def test_long_rows(R, dev, rows, red, offset, dn, omitnan):
    for x in tensors(rows, red, DT[dn][1], 1000 * red + rows):
        check(R, x, dev, dn, omitnan, offset)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_one_row_over_65_chunks(R, dev, dn):
    """2^20 + 3 elements: 65 chunks of 16 Ki elements add into one global histogram"""
    for x in tensors(1, (1 << 20) + 3, DT[dn][1], 77, kinds=('normal', 'nan_one')):
        check(R, x, dev, dn, True)
    for x in tensors(1, (1 << 20) + 3, DT[dn][1], 78, kinds=('zeros_infs',)):
        check(R, x, dev, dn, False)


@pytest.mark.parametrize('dn', ['f32', 'f64'])
@pytest.mark.parametrize('rows,red', [(67, 17), (9, 257), (3, 1025)])
def test_properties(R, dev, rows, red, dn):
    kinds = ('ints', 'normal', 'sorted', 'reversed', 'constant', 'nan_one', 'nan_all_but_one')
    from nitorch_fastmath_amd import _lib
    cap = _lib.lib().nfm_reduce_quantile_max_q()
    for x in tensors(rows, red, DT[dn][1], 5 * red + rows, kinds):
        t = torch.from_numpy(x).to(dev)
        qs = sorted(QLIST)
        for interp in QR.INTERPS:
            v = R.nanquantile(t, qs, dim=1, interpolation=interp).cpu().numpy()
            assert not np.isnan(v).any() and (np.diff(v, axis=0) >= 0).all(), interp          # non-decreasing in q
            assert same_bits(v[0], R.nanmin(t, dim=1).cpu().numpy())                           # q = 0
            assert same_bits(v[-1], R.nanmax(t, dim=1).cpu().numpy())                          # q = 1
        # a q list longer than one launch takes: the same bits as one call per q
        many = [k / (2 * cap + 2) for k in range(2 * cap + 3)]
        for omitnan in (False, True):
            v = R.quantile(t, many, dim=1, omitnan=omitnan)
            assert v.shape == (len(many), rows)
            for k, q in enumerate(many):
                assert same_bits(v[k].cpu().numpy(), R.quantile(t, q, dim=1, omitnan=omitnan).cpu().numpy()), (k, q)


def test_dim_handling(R, dev):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 7, 11)).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.nan
    t = torch.from_numpy(x).to(dev)
    qs = [0.1, 0.5, 0.77]

    def want(rows2d, interp, omitnan):
        return QR.as_dtype(QR.quantiles(rows2d, qs, omitnan)[interp][0], np.float32)
    for omitnan in (False, True):
        for interp in ('lower', 'nearest', 'higher'):
            kw = dict(omitnan=omitnan, interpolation=interp)
            g = R.quantile(t, qs, **kw)                                          # dim=None
            assert g.shape == (3,) and np.array_equal(g.cpu().numpy(), want(x.reshape(1, -1), interp, omitnan)[:, 0], True)
            g = R.quantile(t, qs, dim=[0, 2], **kw)
            assert g.shape == (3, 7)
            assert np.array_equal(g.cpu().numpy(), want(x.transpose(1, 0, 2).reshape(7, 55), interp, omitnan), True)
            g = R.quantile(t, qs, dim=[2, 0], keepdim=True, **kw)                # the order of the dims within a row: free
            assert g.shape == (3, 1, 7, 1)
            assert np.array_equal(g.cpu().numpy().reshape(3, 7), want(x.transpose(1, 0, 2).reshape(7, 55), interp, omitnan), True)
            g = R.quantile(t, qs, dim=1, keepdim=True, **kw)
            assert g.shape == (3, 5, 1, 11)
            w = want(x.transpose(0, 2, 1).reshape(55, 7), interp, omitnan).reshape(3, 5, 1, 11)
            assert np.array_equal(g.cpu().numpy(), w, True)
            g = R.quantile(t, 0.5, dim=-2, **kw)                                 # a scalar q, a negative dim
            assert g.shape == (5, 11) and np.array_equal(g.cpu().numpy(), w[1, :, 0], True)
    # the channel-last VIEW of a channel-first tensor, reduced over the channels
    cf = torch.from_numpy(rng.standard_normal((2, 6, 4, 5))).to(dev)
    cl = cf.permute(0, 2, 3, 1)
    assert not cl.is_contiguous()
    a = R.quantile(cl, [0.2, 0.9], dim=-1)
    assert a.shape == (2, 2, 4, 5) and torch.equal(a, R.quantile(cf, [0.2, 0.9], dim=1))
    m = QR.quantiles(cf.cpu().numpy().transpose(0, 2, 3, 1).reshape(40, 6), [0.2, 0.9], False)['linear']
    assert QR.worst_ratio(a.reshape(2, 40).cpu().numpy(), m[0], m[1], m[2], 2.0 ** -52) <= 4.0
    # out=
    out = torch.empty(0, device=dev)
    r = R.quantile(t, qs, dim=1, out=out)
    assert r is out and out.shape == (3, 5, 11) and same_bits(out.cpu().numpy(), R.quantile(t, qs, dim=1).cpu().numpy())
    with pytest.raises(IndexError):
        R.quantile(torch.empty(3, 0, device=dev), 0.5, dim=1)
    # a device q is copied to the host (a synchronisation): the same result
    qd = torch.tensor(qs, device=dev, dtype=torch.float64)
    assert same_bits(R.quantile(t, qd, dim=1).cpu().numpy(), R.quantile(t, qs, dim=1).cpu().numpy())


def distinct(rows, n, rng):
    """rows of n values at least 0.0075 apart, shuffled: finite differences never reorder them"""
    return np.stack([(rng.permutation(n) + 0.25 * rng.random(n)) * 0.01 for _ in range(rows)])


@pytest.mark.parametrize('interp', ['linear', 'lower'])
@pytest.mark.parametrize('rows,n', [(2, 7), (2, 40), (1, 1100)])
def test_autograd(R, dev, rows, n, interp):
    rng = np.random.default_rng(n)
    x = distinct(rows, n, rng)
    qs = [0.3, 0.62]
    t = torch.from_numpy(x).to(dev).requires_grad_()
    assert torch.autograd.gradcheck(lambda z: R.quantile(z, qs, dim=1, interpolation=interp), (t,), eps=1e-6, atol=1e-7)
    g = torch.from_numpy(rng.standard_normal((2, rows)))
    y = R.quantile(t, qs, dim=1, interpolation=interp)
    (gx,) = torch.autograd.grad(y, t, g.to(dev))
    c = torch.from_numpy(x).requires_grad_()
    yc = torch.quantile(c, torch.tensor(qs, dtype=torch.float64), dim=1, interpolation=interp)
    (gc,) = torch.autograd.grad(yc, c, g)
    assert float((y.detach().cpu() - yc.detach()).abs().max()) <= 1e-12
    assert float((gx.cpu() - gc).abs().max()) <= 1e-12
    with torch.no_grad():                                   # the values of the two routes agree bit for bit
        assert torch.equal(y.detach(), R.quantile(t, qs, dim=1, interpolation=interp))
    with pytest.raises(RuntimeError, match='out='):
        R.quantile(t, qs, dim=1, out=torch.empty(2, rows, device=dev, dtype=torch.float64))


def test_autograd_ties_and_nan_rows(R, dev):
    """among tied elements the gradient goes to the first position holding the value; NaN results carry none"""
    x = torch.tensor([[2.0, 1.0, 2.0, 1.0, 3.0], [1.0, float('nan'), 0.0, 5.0, 4.0]], dtype=torch.float64, device=dev)
    t = x.clone().requires_grad_()
    R.quantile(t, 0.375, dim=1).sum().backward()            # p = 1.5: between ranks 1 and 2 -> values 1 and 2
    assert torch.equal(t.grad, torch.tensor([[0.5, 0.5, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=torch.float64, device=dev))
    t = x.clone().requires_grad_()
    y = R.nanquantile(t, 0.5, dim=1)                        # row 1: count 4, p = 1.5 -> (1 + 4) / 2
    assert y.tolist() == [2.0, 2.5]
    y.sum().backward()
    assert torch.equal(t.grad, torch.tensor([[1.0, 0, 0, 0, 0], [0.5, 0, 0, 0, 0.5]], dtype=torch.float64, device=dev))


def test_graph_capture(R, dev):
    qs = [0.1, 0.5, 0.9]
    for shape in ((9, 257), (1, 40000)):
        x = torch.randn(shape, device=dev)
        eager = R.quantile(x, qs, dim=1)                    # warm-up outside the capture (module load)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = R.quantile(x, qs, dim=1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        x.copy_(torch.randn(shape, device=dev) * 3 + 1)     # new data in the same buffer
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, R.quantile(x, qs, dim=1))
