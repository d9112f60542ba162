"""The yardstick of test_nonfinite_gpu.py, kept honest without a GPU: on every case of nonfinite_cases.py the fp64 restatement
classifies its outputs (finite / +inf / -inf / NaN) as torch's own operator does in fp64 - F.conv2d + F.relu, F.max_pool2d with
the three geometries, F.adaptive_avg_pool2d, F.interpolate with align_corners=True / False / antialias=True - and every case is
shown to do what its name says ON THE REFERENCE: a 'must reach' case has a non-finite output and at least half of its outputs
finite, a 'must not reach' case has none.  So no GPU comparison can pass because nothing was there to compare."""
import pytest
import torch
import torch.nn.functional as F

import classify_reference as CR
import deeplab_reference as DR
import lpips_reference as LR
import nonfinite_cases as NF
import segment_reference as SR


def test_classes_and_poison():
    t = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4e38, -1e-45])
    assert NF.classes(t).tolist() == [0, 0, 1, 2, 3, 0, 0] and NF.classes(t).dtype == torch.int8
    assert NF.classes(t.double()).tolist() == NF.classes(t).tolist()
    x = torch.zeros(2, 3, 4, 5)
    y = NF.poison(x, [((1, 2, 3, 4), "nan"), ((0, 1, slice(0, 2), slice(None)), "ninf"), ((0, 0, 0, 0), 7.0)])
    assert float(x.abs().sum()) == 0.0                                  # a copy
    assert int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(y[1, 2, 3, 4])) and int((y == float("-inf")).sum()) == 10 and float(y[0, 0, 0, 0]) == 7.0
    assert NF.is_subset(NF.classes(torch.tensor([0.0, float("nan")])), NF.classes(torch.tensor([float("inf"), float("nan")])))
    assert NF.is_subset(NF.classes(torch.tensor([float("inf"), 0.0])), NF.classes(torch.tensor([float("nan"), 0.0])))      # 0 x inf
    assert not NF.is_subset(NF.classes(torch.tensor([float("nan"), 0.0])), NF.classes(torch.tensor([float("inf"), 0.0])))
    assert not NF.is_subset(NF.classes(torch.tensor([float("inf"), 0.0])), NF.classes(torch.tensor([float("-inf"), 0.0])))
    assert not NF.is_subset(NF.classes(torch.tensor([float("inf"), 0.0])), NF.classes(torch.tensor([0.0, 0.0])))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "no_relu"])
@pytest.mark.parametrize("value", NF.VALUE_NAMES)
@pytest.mark.parametrize("name", sorted(NF.CONV_NONFINITE))
def test_conv_restatement_classifies_as_torch(name, value, relu):
    case, clean, want, bound = NF.conv_case(name, value, relu)
    assert torch.equal(NF.classes(want), NF.classes(NF.conv_torch(case, relu)))
    reach, clean_images = NF.CONV_NONFINITE[name][3:5]
    if reach and not (relu and value == "ninf" and NF.CONV_NONFINITE[name][1] == "res"):
        # (a -inf residual under the ReLU is 0: that case checks that nothing non-finite comes out)
        NF.reach_conditions(want, True)
    else:
        NF.reach_conditions(want, False)
    # the bound is finite wherever the reference is, and the clean images' outputs are those of the clean input
    assert bool(torch.isfinite(bound[NF.classes(want) == NF.FINITE]).all())
    want_clean = DR.conv(clean["x"], clean["w"], clean["b"], clean["stride"], clean["pad"], clean["dil"], clean["res"], relu)
    for i in clean_images:
        assert torch.equal(want[i], want_clean[i])
    if relu:                                                            # torch.relu keeps NaN and +inf, and turns -inf into 0
        assert not bool((want == float("-inf")).any())


def test_relu_and_max_pool_of_torch_keep_nan():
    """The two facts the kernels' contract rests on, asked of torch itself."""
    nan = float("nan")
    assert bool(torch.isnan(torch.relu(torch.tensor(nan)))) and float(torch.relu(torch.tensor(float("-inf")))) == 0.0
    x = torch.tensor([[nan, 1.0, 2.0], [3.0, 4.0, 5.0], [6.0, 7.0, 8.0]]).view(1, 1, 3, 3)
    for flip in (False, True):                                          # the first tap and the last
        assert bool(torch.isnan(F.max_pool2d(x.flip(2, 3) if flip else x, kernel_size=3, stride=2)).all())
    assert float(F.max_pool2d(torch.full((1, 1, 3, 3), float("-inf")), kernel_size=3, stride=2)) == float("-inf")


@pytest.mark.parametrize("run", NF.pool_runs(), ids=[r[0] for r in NF.pool_runs()])
def test_pool_restatement_classifies_as_torch(run):
    _id, name, value = run
    kind, x, clean, want = NF.pool_case(name, value)
    theirs = NF.POOLS[kind][2](x.double())
    assert torch.equal(NF.classes(want), NF.classes(theirs))
    ok = NF.classes(want) == NF.FINITE
    assert torch.equal(want[ok].double(), theirs[ok])                   # a max is exact: the finite values are torch's
    NF.reach_conditions(want, NF.pool_reaches(name, value))
    if not NF.POOL_NONFINITE[name][3]:
        assert torch.equal(want, NF.POOLS[kind][1](clean))              # the value is never read
    if "all_ninf" in name:
        assert set(NF.classes(want).unique().tolist()) == {NF.FINITE, NF.NINF}
    if "pinf_and_ninf" in name:
        assert NF.NINF not in NF.classes(want).unique().tolist() and NF.PINF in NF.classes(want).unique().tolist()


def test_one_nan_reaches_1_1_and_9_outputs_of_the_three_pools():
    """One NaN at an even interior coordinate of a 9 x 9 map: 4 windows of the unpadded 3x3 / 2 pool hold it, 1 of the padded one
    and 25 of the 5x5 / 1 pool; at an odd coordinate 1, 4 and 25."""
    for pos, counts in (((4, 4), (4, 1, 25)), ((3, 3), (1, 4, 25))):
        x = NF.poison(torch.zeros(1, 1, 9, 9), [((0, 0, *pos), "nan")])
        got = tuple(int(torch.isnan(f(x)).sum()) for f in (LR.pool, CR.maxpool, SR.maxpool5))
        assert got == counts


@pytest.mark.parametrize("run", NF.avgpool_runs(), ids=[r[0] for r in NF.avgpool_runs()])
def test_avgpool_restatement_classifies_as_torch(run):
    _id, name, value = run
    x, _clean, want = NF.avgpool_case(name, value)
    theirs = F.adaptive_avg_pool2d(x.double(), 1)[:, :, 0, 0]
    assert torch.equal(NF.classes(want), NF.classes(theirs))
    NF.reach_conditions(want, True)
    (n, c, *_), _v = NF.AVGPOOL_NONFINITE[name][1][0]
    bad = NF.classes(want) != NF.FINITE
    assert int(bad.sum()) == 1 and bool(bad[n, c])                      # exactly the poisoned (image, channel)
    if "pinf_and_ninf" in name:
        assert int(NF.classes(want)[n, c]) == NF.NAN


@pytest.mark.parametrize("value", NF.VALUE_NAMES)
@pytest.mark.parametrize("shape", NF.ADD_SHAPES, ids=["x".join(map(str, s)) for s in NF.ADD_SHAPES])
def test_add_restatement(shape, value):
    a, b, want = NF.add_case(shape, value)
    assert torch.equal(NF.classes(want), NF.classes(torch.add(a.double(), b.double())))
    NF.reach_conditions(want, True)
    assert int(NF.classes(want)[0, 1, 2, 3]) == NF.NAN                  # +inf on -inf
    assert int((NF.classes(want) != NF.FINITE).sum()) == 3


@pytest.mark.parametrize("value", NF.VALUE_NAMES)
@pytest.mark.parametrize("name", sorted(NF.RESIZE_NONFINITE))
def test_resize_restatement_holds_torchs_pattern(name, value):
    """`resize_tables` against F.interpolate in fp64: the same values where both are finite (to fp64 rounding), and torch's
    non-finite pattern is a SUBSET of the restatement's - not equal to it, for the reason nonfinite_cases.py gives: an output that
    sits on a source sample takes the weights (1, 0) from the exact tables and so reads a non-finite right / lower neighbour,
    while torch's floating-point split may land below the sample and read the left / upper one, and torch does not always
    multiply a clamped tap by its zero weight (an infinity then stays one where the tables give 0 x inf = NaN).  Where they
    differ the restatement is the authority (it is what `bilerp` documents); the count of such outputs is printed."""
    table, size, x, clean, want, _bound = NF.resize_case(name, value)
    theirs = NF.resize_torch(x, size, table)
    k_want, k_theirs = NF.classes(want), NF.classes(theirs)
    assert NF.is_subset(k_theirs, k_want)
    extra = int((k_want != k_theirs).sum())
    print(f"{name} {value}: {int((k_want != NF.FINITE).sum())} non-finite outputs, {extra} of them of another class in torch")
    assert value != "nan" or extra == 0                                 # a NaN reaches the same outputs in both
    both = (k_want == NF.FINITE) & (k_theirs == NF.FINITE)
    assert float((want[both] - theirs[both]).abs().max()) <= 1e-14 * float(clean.abs().max())
    # on the clean input the restatement IS torch's resize
    assert float((NF.resize_tables(clean, size, table) - NF.resize_torch(clean, size, table)).abs().max()) <= 1e-14 * float(clean.abs().max())
    NF.reach_conditions(want, True)
    # the value stays in its own image and channel
    n, c = NF.RESIZE_NONFINITE[name][2][:2]
    bad = k_want != NF.FINITE
    assert int(bad.sum()) == int(bad[n, c].sum())


@pytest.mark.parametrize("value", NF.VALUE_NAMES)
def test_preprocess_restatements_classify_as_torch(value):
    """The metrics' own preprocesses: LPIPS's scaling (pointwise), the classifier's antialiased resize (CR.preprocess IS
    F.interpolate(antialias=True) + Normalize) and the two segmenters' (SR.prep / DR.prep are F.interpolate(align_corners=True)
    + their arithmetic)."""
    x = NF.poison(LR.images(NF.LPIPS_PREP_SHAPE, 3)[0], [(NF.IMAGE_POSITION, value)])
    want = LR.scale_input(x)
    assert int((NF.classes(want) != NF.FINITE).sum()) == 1 and int(NF.classes(want)[NF.IMAGE_POSITION]) == NF.classes(x)[NF.IMAGE_POSITION]
    x = NF.poison(CR.images(NF.CLASSIFY_PREP_SHAPE, 5), [(NF.IMAGE_POSITION, value)])
    want = CR.preprocess(x)
    theirs = F.interpolate(x.double(), size=(224, 224), mode="bilinear", antialias=True, align_corners=False)
    assert torch.equal(NF.classes(want), NF.classes(theirs))
    NF.reach_conditions(want, True)
    assert int((NF.classes(want[0]) != NF.FINITE).sum()) == 0           # image 0 is clean
    for R in (SR, DR):
        shape, s = R.PREP_CASES[0]
        size = R.scaled_hw(shape[2], shape[3], s)
        x = NF.poison(R.images(shape, sum(shape)), [((0, 1, 9, 13), value)])
        want = R.prep(x, size)
        theirs = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=True)
        if R is SR:
            theirs = theirs.flip(1)                                     # RefineNet-LW's input is B, G, R
        assert torch.equal(NF.classes(want), NF.classes(theirs))
        NF.reach_conditions(want, True)


def test_host_metrics_of_a_poisoned_image_are_nan():
    """runner.psnr_per_image / runner.ssim, the authority of ops.image_metrics: NaN for the poisoned image, the clean values for
    the others."""
    from unirestore_amd import runner
    pred, tgt = LR.images((3, 3, 20, 24), 8)
    bad = NF.poison(pred, [(NF.IMAGE_POSITION, "nan")])
    ps, ps_clean = runner.psnr_per_image(bad, tgt), runner.psnr_per_image(pred, tgt)
    assert NF.classes(ps).tolist() == [0, 3, 0] and torch.equal(ps[[0, 2]], ps_clean[[0, 2]])
    for i in range(3):
        s = runner.ssim(bad[i:i + 1], tgt[i:i + 1])
        assert (s != s) == (i == 1) and (i == 1 or s == runner.ssim(pred[i:i + 1], tgt[i:i + 1]))
