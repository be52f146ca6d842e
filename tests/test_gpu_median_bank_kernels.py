"""The width-bank median kernel (csrc/median_bank.hip) alone: every slice bit for bit against `ops.detect_median` at that
width and against the restatement of tests/median_bank_ref.py.  The tables are those of tests/test_gpu_detect_kernels.py:
recordings of every awkward length side by side plus two constant neighbours, inputs in tenths so that ties are frequent.
The output is pre-filled with NaN, every element must come back finite, and a second call must agree bit for bit.  A
selection has no tolerance: everything is compared for equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops  # noqa: E402
from efficientat_amd._lib import EatHipError  # noqa: E402
from tests.median_bank_ref import median_bank_ref  # noqa: E402

DEV = torch.device("cuda:0")
LENGTHS = [1, 2, 15, 16, 31, 64, 65, 1000]
ALL_ODD = np.arange(1, 32, 2)


def _rec(lengths):
    out, goff = [], 0
    for i, G in enumerate(lengths):
        out.append((i, 1, goff, G))
        goff += G
    return out


def _tenths(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 11, shape, generator=g).float() / 10.0


def _side_by_side(K, seed):
    """-> (x (K, G_total), rec, first column of the two constant 20-frame neighbours at 0.1 and 0.9)."""
    rec = _rec(LENGTHS + [20, 20])
    x = _tenths((K, sum(r[3] for r in rec)), seed)
    lo0 = rec[-2][2]
    x[:, lo0:lo0 + 20] = 0.1
    x[:, lo0 + 20:] = 0.9
    return x, rec, lo0


def _bank_case(x, rec, widths):
    """One call into a NaN-filled buffer and one into a fresh one -> (filt on the host, the restatement)."""
    widths = np.atleast_2d(np.asarray(widths))
    table = ops.detect_table(rec)
    wt = ops.median_width_table(widths, x.shape[0])
    d_x = x.to(DEV)
    out = torch.full((wt.Mw,) + tuple(x.shape), float("nan"), device=DEV)
    got = ops.detect_median_bank(d_x, table, wt, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (wt.Mw,) + tuple(x.shape)
    again = ops.detect_median_bank(d_x, table, widths)                        # (a plain array is validated on the way)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, again)
    assert torch.equal(d_x.cpu(), x)                                          # the input is left alone
    return got.cpu(), torch.from_numpy(median_bank_ref(x.numpy(), rec, widths))


@pytest.mark.parametrize("K", [1, 5, 527])
def test_constant_widths_per_slice_equal_detect_median(K):
    x, rec, lo0 = _side_by_side(K, seed=K)
    ms = (1, 3, 5, 31)
    got, want = _bank_case(x, rec, np.repeat(np.asarray(ms)[:, None], K, axis=1))
    table, d_x = ops.detect_table(rec), x.to(DEV)
    for j, m in enumerate(ms):
        single = ops.detect_median(d_x, table, m).cpu()
        print(f"bank K={K} m={m}: {int((got[j] != single).sum())} elements differ from detect_median, "
              f"{int((got[j] != want[j]).sum())} from the restatement, of {single.numel()}")
        assert torch.equal(got[j], single)
        assert torch.equal(got[j], want[j])
        assert torch.equal(got[j][:, lo0:], x[:, lo0:])                       # constant recordings stay what they are
    assert torch.equal(got[0], x)                                             # width 1 is a copy


@pytest.mark.parametrize("K", [1, 5, 527])
def test_random_widths_per_class_in_one_slice(K):
    x, rec, lo0 = _side_by_side(K, seed=100 + K)
    widths = np.random.default_rng(K).choice([1, 3, 5, 7, 31], size=(1, K))
    got, want = _bank_case(x, rec, widths)
    print(f"bank per-class widths K={K}: {int((got != want).sum())} of {want.numel()} elements differ; widths used "
          f"{sorted(set(widths.reshape(-1).tolist()))}")
    assert torch.equal(got, want)
    assert torch.equal(got[0][:, lo0:], x[:, lo0:])
    ones = np.flatnonzero(widths[0] == 1)
    assert torch.equal(got[0][ones], x[ones])


def _permuted(K, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(ALL_ODD) for _ in range(K)], axis=1)     # (16, K): every class has every width once


@pytest.mark.parametrize("K", [1, 5, 527])
def test_all_widths_in_an_order_permuted_per_class(K):
    """The halo staged is the class's widest, 31, and the slices of one class disagree about theirs."""
    x, rec, lo0 = _side_by_side(K, seed=200 + K)
    widths = _permuted(K, K)
    assert widths.shape == (16, K) and all(sorted(widths[:, k].tolist()) == ALL_ODD.tolist() for k in range(K))
    got, want = _bank_case(x, rec, widths)
    print(f"bank all widths K={K}: {int((got != want).sum())} of {want.numel()} elements differ")
    assert torch.equal(got, want)
    assert torch.equal(got[:, :, lo0:], x[:, lo0:].expand(16, -1, -1))


@pytest.mark.parametrize("G", [255, 256, 257, 513])
def test_one_recording_whose_halo_crosses_a_tile_edge(G):
    x = _tenths((3, G), seed=G)
    got, want = _bank_case(x, _rec([G]), [[3, 31, 3], [31, 3, 1]])
    print(f"bank G={G}: {int((got != want).sum())} of {want.numel()} elements differ")
    assert torch.equal(got, want)


@pytest.mark.parametrize("G", [1, 2])
def test_reflection_wraps_several_times(G):
    x = _tenths((3, G), seed=7 + G)
    got, want = _bank_case(x, _rec([G]), [[31, 31, 1], [3, 5, 31]])
    assert torch.equal(got, want)
    if G == 1:
        assert torch.equal(got, x.expand(2, -1, -1))


def test_refusals():
    x = _tenths((2, 40), seed=1).to(DEV)
    table = ops.detect_table([(0, 1, 0, 40)])
    for bad in (2, 0, 33):
        with pytest.raises(EatHipError, match=f"slice 0, class 1: width {bad} "):
            ops.detect_median_bank(x, table, [[3, bad]])
    with pytest.raises(EatHipError, match="K = 2"):
        ops.detect_median_bank(x, table, np.ones((2, 3), dtype=np.int64))     # an (Mw, K + 1) table
    with pytest.raises(EatHipError, match="holds 3 classes, prob 2"):
        ops.detect_median_bank(x, table, ops.median_width_table([1, 3, 5], 3))
    with pytest.raises(EatHipError, match="integers"):
        ops.detect_median_bank(x, table, [[3.0, 5.0]])
    with pytest.raises(EatHipError, match="Mw >= 1"):
        ops.detect_median_bank(x, table, np.ones((0, 2), dtype=np.int64))     # Mw = 0
    buf = torch.zeros(200, device=DEV)
    with pytest.raises(EatHipError, match="out must not overlap prob"):
        ops.detect_median_bank(buf[:80].view(2, 40), table, [[3, 3], [5, 5]], out=buf[40:].view(2, 2, 40))
    with pytest.raises(EatHipError, match="out must not overlap prob"):
        ops.detect_median_bank(x, table, [3, 3], out=x)
    with pytest.raises(EatHipError, match="GPU"):
        ops.detect_median_bank(x.cpu(), table, [3, 3])
    # the library's own check, behind the Python one
    from efficientat_amd import _lib
    w = ops.median_width_table([3, 3], 2).dev(DEV)
    with pytest.raises(EatHipError, match="Mw >= 1"):
        _lib.call("eat_detect_median_bank", x.data_ptr(), 2, 40, table.dev(DEV).data_ptr(), 1, w.data_ptr(), 0, buf.data_ptr(), None)
    with pytest.raises(EatHipError, match="filt must not be prob"):
        _lib.call("eat_detect_median_bank", x.data_ptr(), 2, 40, table.dev(DEV).data_ptr(), 1, w.data_ptr(), 1, x.data_ptr(), None)
    with pytest.raises(EatHipError, match="missing operand"):
        _lib.call("eat_detect_median_bank", x.data_ptr(), 2, 40, table.dev(DEV).data_ptr(), 1, None, 1, buf.data_ptr(), None)


def test_index_past_2_to_31():
    """(Mw, K, G_total) = (16, 33, 2^22 + 37): 2.2e9 output elements, the last 16 class rows of the last slice wholly beyond a
    32-bit element index, while K G_total itself stays far below it."""
    Mw, K, G_a, G_b = 16, 33, 2 ** 22, 37
    G_total = G_a + G_b
    need = 4 * (Mw + 1) * K * G_total + 2 ** 30                               # filt, prob and a GB to spare
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < need:
        pytest.skip(f"{free / 2 ** 30:.1f} GB of device memory free: the buffers need {need / 2 ** 30:.1f}")
    rec = _rec([G_a, G_b])
    table = ops.detect_table(rec)
    assert K * G_total < 2 ** 31 < (Mw * K - 1) * G_total                     # row K - 1 of the last slice starts beyond it
    widths = _permuted(K, 9)
    prob = torch.randint(0, 11, (K, G_total), device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)).float() / 10.0
    filt = ops.detect_median_bank(prob, table, widths)
    assert filt.shape == (Mw, K, G_total)
    for j in (0, Mw - 1):
        for k in (0, K - 1):
            m = int(widths[j, k])
            head = prob[k, :600].cpu().numpy()[None, :]                       # 88 columns of context: more than any halo
            assert np.array_equal(filt[j, k, :512].cpu().numpy(), median_bank_ref(head, [(0, 1, 0, 600)], [m])[0, 0, :512]), (j, k)
            end = prob[k, G_a - 600:G_a].cpu().numpy()[None, :]
            assert np.array_equal(filt[j, k, G_a - 512:G_a].cpu().numpy(),
                                  median_bank_ref(end, [(0, 1, 0, 600)], [m])[0, 0, 88:]), (j, k)
            last = prob[k, G_a:].cpu().numpy()[None, :]
            assert np.array_equal(filt[j, k, G_a:].cpu().numpy(), median_bank_ref(last, [(0, 1, 0, G_b)], [m])[0, 0]), (j, k)
    del prob, filt
    torch.cuda.empty_cache()
