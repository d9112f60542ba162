"""NIQE, the parts that need no GPU: the tables, NaN handling, the parameter files, every --niqe argument error, the condition
that makes the exact comparison of alpha indices legitimate, and the GPU tolerances of niqe_cases.py against what the two
summation orders of niqe_reference.py measure here."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

import niqe_cases as C
import niqe_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- table values ----------------------------------------------------------------------------------------------------------------

def test_halve_taps_are_the_stretched_cubic_kernel():
    from unirestore_amd import niqe
    derived = R.halve_taps_from_kernel()
    assert list(niqe.HALVE_TAPS) == list(R.HALVE_TAPS) == derived                 # exact in binary
    assert sum(niqe.HALVE_TAPS) == 1.0


def test_gaussian_sums_to_one():
    from unirestore_amd import niqe
    g = niqe.gaussian7()
    assert len(g) == 7 and g == g[::-1] and abs(sum(g) - 1.0) < 1e-15
    k = torch.tensor(R.gaussian2d(), dtype=torch.float64)
    assert abs(float(k.sum()) - 1.0) < 1e-15
    g64 = torch.tensor(g, dtype=torch.float64)
    assert float((k - torch.outer(g64, g64)).abs().max()) < 1e-15               # the separable form is the same window


def test_alpha_grid_and_rho_table():
    from unirestore_amd import niqe
    alpha, rho, scale, ratio = niqe.alpha_tables()
    assert niqe.GRID == 9801 and alpha.numel() == rho.numel() == scale.numel() == ratio.numel() == 9801
    assert float(alpha[0]) == 0.2 and abs(float(alpha[-1]) - 10.0) < 1e-12
    assert np.array_equal(alpha.numpy(), 0.2 + 0.001 * np.arange(9801))
    assert bool((rho[1:] > rho[:-1]).all())                                       # strictly increasing: bisection is legitimate
    for t, u in zip((alpha, rho, scale, ratio), R.tables()):
        assert torch.equal(t, u)
    a = 2.0                                                                         # a Gaussian: rho = 2 / pi
    i = 1800
    assert abs(float(alpha[i]) - a) < 1e-12 and abs(float(rho[i]) - 2 / math.pi) < 1e-12
    assert abs(float(scale[i]) - math.sqrt(math.gamma(0.5) / math.gamma(1.5))) < 1e-15


# ---- NaN handling ----------------------------------------------------------------------------------------------------------------

def test_zero_counts_give_nan_features():
    good = [4000.0, 900.0, 5216.0, 1500.0, 2500.0, 2400.0]
    mom = torch.tensor([[good, good, good, good, good],
                        [[0.0, 0.0, 9216.0, 1500.0, 2500.0, 1500.0], good, good, good, good],            # no negative entry in M
                        [good, [4000.0, 900.0, 0.0, 0.0, 1500.0, 900.0], good, good, good],                # no positive one in a product
                        [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0]] * 5], dtype=torch.float64)[None]                # a flat block
    feat, idx = R.fit(mom, 96 * 96)
    nan = torch.isnan(feat[0])
    assert not nan[0].any() and (idx[0, 0] >= 0).all()
    assert nan[1, :2].all() and not nan[1, 2:].any() and idx[0, 1].tolist()[0] == -1
    assert nan[2, 2:6].all() and not nan[2, :2].any() and not nan[2, 6:].any() and idx[0, 2].tolist()[1] == -1
    assert nan[3].all() and (idx[0, 3] == -1).all()


def test_score_uses_nanmean_and_drops_nan_rows():
    from unirestore_amd import niqe
    g = torch.Generator().manual_seed(3)
    rows = torch.randn(5, 36, generator=g, dtype=torch.float64)
    rows[1, 7] = float("nan")
    mu_p, cov_p = C.params_host()
    p = niqe.NiqeParams(mu_p, cov_p, dev="cpu")
    got = niqe.score(rows[None], p)
    good = rows[[0, 2, 3, 4]]
    mu = rows.clone()
    mu[1, 7] = 0.0
    mu = mu.sum(0) / torch.tensor([4.0 if j == 7 else 5.0 for j in range(36)], dtype=torch.float64)       # nanmean: row 1 still counts elsewhere
    cov = torch.from_numpy(np.cov(good.numpy().T, ddof=1))
    d = mu_p - mu
    want = torch.sqrt(d @ torch.linalg.pinv((cov_p + cov) / 2) @ d)
    assert got.shape == (1,) and got.dtype == torch.float64 and abs(float(got[0]) - float(want)) < 1e-12 * float(want)
    assert abs(float(R.score(rows[None], mu_p, cov_p)[0]) - float(want)) < 1e-12 * float(want)
    assert float(niqe.score(rows, p)[0]) == float(got[0])                          # one image's [blocks, 36]
    two = rows[:3].clone()                                                          # rows 0 and 2 are good: still a score
    assert bool(torch.isfinite(niqe.score(two[None], p)).all())
    one = two.clone()
    one[2, 0] = float("nan")                                                        # one good row: no covariance, NaN
    assert bool(torch.isnan(niqe.score(one[None], p)).all()) and bool(torch.isnan(R.score(one[None], mu_p, cov_p)).all())
    both = niqe.score(torch.stack([two, one]), p)
    assert bool(torch.isfinite(both[0])) and bool(torch.isnan(both[1]))


# ---- parameter files -------------------------------------------------------------------------------------------------------------

def test_params_round_trip_pt_and_npz(tmp_path):
    from unirestore_amd import niqe
    mu, cov = C.params_host()
    torch.save({"mu_prisparam": mu.reshape(1, 36), "cov_prisparam": cov}, tmp_path / "p.pt")
    torch.save({"mu_prisparam": mu.float(), "cov_prisparam": cov.float()}, tmp_path / "p.pth")
    np.savez(tmp_path / "p.npz", mu_prisparam=mu.numpy().reshape(1, 36), cov_prisparam=cov.numpy())
    for name, exact in (("p.pt", True), ("p.npz", True), ("p.pth", False)):
        p = niqe.load_params(str(tmp_path / name), dev="cpu")
        assert p.mu.shape == (36,) and p.cov.shape == (36, 36) and p.mu.dtype == p.cov.dtype == torch.float64
        assert p.device == torch.device("cpu")
        if exact:
            assert torch.equal(p.mu, mu) and torch.equal(p.cov, cov)
        else:
            assert torch.equal(p.mu, mu.float().double())
    r = niqe.random_params(4, dev="cpu")
    assert torch.equal(r.cov, r.cov.T) and float(torch.linalg.eigvalsh(r.cov).min()) > 0
    assert torch.equal(niqe.random_params(4, dev="cpu").mu, r.mu) and not torch.equal(niqe.random_params(5, dev="cpu").mu, r.mu)
    assert "ONLY" in niqe.random_params.__doc__ and "NOT applied" in niqe.fit_params.__doc__


def test_params_round_trip_mat(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from unirestore_amd import niqe
    mu, cov = C.params_host()
    sio.savemat(str(tmp_path / "niqe_modelparameters.mat"), {"mu_prisparam": mu.numpy().reshape(1, 36), "cov_prisparam": cov.numpy()})
    p = niqe.load_params(str(tmp_path / "niqe_modelparameters.mat"), dev="cpu")
    assert torch.equal(p.mu, mu) and torch.equal(p.cov, cov)


def test_mat_without_scipy_names_scipy(tmp_path, monkeypatch):
    import builtins
    from unirestore_amd import niqe
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.split(".")[0] == "scipy":
            raise ImportError("No module named 'scipy'")
        return real(name, *a, **k)
    (tmp_path / "m.mat").write_bytes(b"")
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(ImportError, match="scipy"):
        niqe.load_params(str(tmp_path / "m.mat"), dev="cpu")


def test_every_params_error_names_source_and_key(tmp_path):
    from unirestore_amd import niqe
    mu, cov = C.params_host()
    bad_mu, bad_cov = mu.clone(), cov.clone()
    bad_mu[3] = float("inf")
    bad_cov[2, 2] = float("nan")
    for m, c, words in ((mu[:35], cov, ("mu_prisparam", "(35,)")), (mu.reshape(36, 1), cov, ("mu_prisparam", "(36, 1)")),
                        (mu, cov[:, :35], ("cov_prisparam", "(36, 35)")), (mu, cov.reshape(-1), ("cov_prisparam", "(1296,)")),
                        (bad_mu, cov, ("mu_prisparam", "non-finite")), (mu, bad_cov, ("cov_prisparam", "non-finite")),
                        ("text", cov, ("mu_prisparam", "numeric"))):
        with pytest.raises(ValueError) as e:
            niqe.NiqeParams(m, c, dev="cpu", source="SRC")
        assert "SRC" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    torch.save({"mu_prisparam": mu}, tmp_path / "nocov.pt")
    with pytest.raises(ValueError, match="cov_prisparam") as e:
        niqe.load_params(str(tmp_path / "nocov.pt"), dev="cpu")
    assert "nocov.pt" in str(e.value)
    torch.save([mu, cov], tmp_path / "list.pt")
    with pytest.raises(ValueError, match="list.pt"):
        niqe.load_params(str(tmp_path / "list.pt"), dev="cpu")
    with pytest.raises(ValueError, match="extension"):
        niqe.load_params(str(tmp_path / "p.json"), dev="cpu")
    assert niqe.BLOCK == 96 and niqe.MIN_BLOCKS == 2 and niqe.COLOR_SPACES == ("yiq", "ycbcr")


# ---- the command line ------------------------------------------------------------------------------------------------------------

class _NoModel:
    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the arguments were checked")


def _params_file(tmp_path, name="p.pt"):
    mu, cov = C.params_host()
    torch.save({"mu_prisparam": mu, "cov_prisparam": cov}, tmp_path / name)
    return str(tmp_path / name)


def test_niqe_argument_errors_come_before_the_model(tmp_path):
    from unirestore_amd import cli
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_256_4step.yaml"))
    good = _params_file(tmp_path)
    assert cli.check_niqe_arg(good) == good
    (tmp_path / "p.json").write_text("{}")
    for arg, crop, word in ((str(tmp_path / "missing.pt"), None, "no such file"), (str(tmp_path / "p.json"), None, "extension"),
                            (5, None, "--niqe takes"), (good, (96, 191), "96 x 191"), (good, "95,400", "95 x 400"),
                            (good, (191, 191), "191 x 191")):
        with pytest.raises(ValueError) as e:
            cli.validate(cfg, niqe=arg, crop=crop, model=_NoModel())
        assert word in str(e.value) and "--niqe" in str(e.value), str(e.value)
    assert inspect.signature(cli.validate).parameters["niqe"].default is None


def test_niqe_flag_belongs_to_validate(tmp_path, capsys):
    from unirestore_amd import cli
    cfg = os.path.join(ROOT, "configs", "val_pir_256_4step.yaml")
    good = _params_file(tmp_path)
    for argv, word in ((["restore", "--config", cfg, "--niqe", good], "--niqe belongs to validate"),
                       (["print_config", "--config", cfg, "--niqe", good], "--niqe belongs to validate"),
                       (["corrupt", "--niqe", good], "--niqe belongs to validate"),
                       (["validate", "--config", cfg, "--niqe", str(tmp_path / "missing.npz")], "no such file"),
                       (["validate", "--config", cfg, "--niqe", good, "--crop", "96,100"], "96 x 100")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, argv


def test_entry_points_refuse_shapes_beyond_their_limits():
    """Checked on the host before any HIP call: a null pointer or a malformed shape is invalid, a shape past a stated limit is
    unsupported - never a wrong launch."""
    from unirestore_amd.capi import UR_E_INVALID, UR_E_UNSUPPORTED, lib
    p = 4096                                                                        # never dereferenced: every call below is refused
    big = 1 << 16
    assert lib.ur_niqe_luma(p, p, 1, big, big, 96 * 600, 96 * 600, 0, None) == UR_E_UNSUPPORTED
    assert lib.ur_niqe_luma(p, p, 1, 96, 96, 192, 96, 0, None) == UR_E_INVALID
    assert lib.ur_niqe_luma(p, p, 1, 96, 96, 96, 96, 2, None) == UR_E_INVALID
    assert lib.ur_niqe_luma(None, p, 1, 96, 96, 96, 96, 0, None) == UR_E_INVALID
    assert lib.ur_niqe_mscn(p, p + 8, 1 << 12, 1 << 15, 1 << 15, None) == UR_E_UNSUPPORTED
    assert lib.ur_niqe_mscn(p, p, 1, 96, 96, None) == UR_E_INVALID
    assert lib.ur_niqe_halve(p, p + 8, 2, big, big, None) == UR_E_UNSUPPORTED
    assert lib.ur_niqe_halve(p, p + 8, 1, 97, 96, None) == UR_E_INVALID
    assert lib.ur_niqe_block_moments(p, p + 8, 1 << 30, 96, 192, 96, None) == UR_E_UNSUPPORTED
    assert lib.ur_niqe_block_moments(p, p + 8, 1, 96, 192, 64, None) == UR_E_INVALID
    assert lib.ur_niqe_block_moments(p, p + 8, 1, 96, 100, 96, None) == UR_E_INVALID
    assert lib.ur_niqe_fit(p, p, p, p, p, None, 1 << 29, 9216, 36, 0, None) == UR_E_UNSUPPORTED
    assert lib.ur_niqe_fit(p, p, p, p, p, None, 1 << 62, 9216, 36, 0, None) == UR_E_UNSUPPORTED
    assert lib.ur_niqe_fit(p, p, p, p, p, None, 4, 9216, 36, 19, None) == UR_E_INVALID
    assert lib.ur_niqe_fit(p, None, p, p, p, None, 4, 9216, 36, 0, None) == UR_E_INVALID


# ---- the alpha indices may be compared exactly -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def measured():
    return {case: C.measure(case) for case in C.CASES}


@pytest.mark.parametrize("case", C.CASES)
def test_ratios_stay_clear_of_the_grid_midpoints(measured, case):
    """An implementation picks the yardstick's alpha while its R stays on the yardstick's side of the midpoint between two rho
    values: every R of every case lies at least 1e-9 (relative) from one, orders of magnitude more than R moves between two
    summation orders, and the two orders do pick the same indices and the same NaNs."""
    m = measured[case]
    print(f"{case}: margin {m['margin']:.3e}, order-to-order difference of R {m['r_diff']:.3e}")
    assert m["margin"] >= C.MIN_MARGIN, m
    assert m["r_diff"] * 1e3 < m["margin"], m
    assert m["same_index"] and m["same_nan"] and m["luma_equal"]
    ref = C.reference(case)
    assert not bool(torch.isnan(ref["features"]).any())                              # no flat block in the cases
    assert bool((ref["index1"] >= 0).all()) and bool((ref["index2"] >= 0).all())


# ---- the tolerances --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.CASES)
def test_stored_tolerances_cover_sixteen_times_the_measurement(measured, case):
    m = measured[case]
    print(case, {q: f"{m[q]:.3e}" for q in C.QUANTITIES})
    for q in C.QUANTITIES:
        assert C.MEASURED[case][q] >= m[q], (case, q, m[q])                           # the record is still an upper bound here
        assert C.tolerance(case, q) >= C.FACTOR * m[q], (case, q, m[q])
        assert C.tolerance(case, q) <= 1e-10                                          # and never a loose one


def test_tolerance_record_matches_the_constants():
    text = open(os.path.join(ROOT, "profiles", "niqe_tolerances.txt")).read()
    for case in C.CASES:
        for q in C.QUANTITIES:
            assert f"{case:<12} {q:<9} {C.MEASURED[case][q]:.2e}  {C.TOLERANCE[case][q]:.3e}" in text, (case, q)


def test_case_shapes():
    shapes = {c: tuple(C.images(c).shape) for c in C.CASES}
    assert shapes == {"two_blocks": (2, 3, 96, 192), "ragged": (2, 3, 200, 301), "unquantised": (3, 3, 192, 192), "ycbcr": (2, 3, 96, 192)}
    for c in ("two_blocks", "ragged", "ycbcr"):
        x = C.images(c).double() * 255
        assert torch.equal(x.round(), (x + 0.0).round()) and float((x - x.round()).abs().max()) < 1e-4      # on the 8-bit grid
    assert C.images("unquantised").dtype == torch.float32
    assert tuple(C.reference("ragged")["luma"].shape) == (2, 192, 288)
