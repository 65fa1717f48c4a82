"""The batch entry points of include/mpc_amd.h, every family in each of its forms (plain, _model, _warm, _warm_model) through the raw
C ABI (tests/entry_point_forms.py): leading dimensions larger than the batch, model = NULL forwarding to the form without _model,
and what each form refuses, with which code and text, in which order.  N = 10 (config-fast.json) unless a row says otherwise.

The table of refusals is E.REFUSALS.  Two of its rows are not what one would guess: the HOST solve forms answer ld = B - 1 and
B = max_batch + 1 with "bad B/ld" (their check is the one of the run() and rollout forms), only the device solve forms with
"ld < B" and "max_batch"."""
import os

import pytest

import entry_point_forms as E

pytestmark = pytest.mark.gpu

CFG = "config-fast.json"


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fast(pkg, golden_dir):
    return pkg.params_from_json(os.path.join(golden_dir, CFG))


@pytest.fixture(scope="module")
def fleet(pkg, fast, waypoints):
    """cars(B), drawn once per B"""
    made = {}

    def get(B):
        if B not in made:
            made[B] = E.cars(pkg, fast, waypoints, B)
        return made[B]
    return get


def _same(a, b, what):
    assert len(a) == len(b), what
    words = 0
    for x, y in zip(a, b):
        assert x["rc"] == 0 and y["rc"] == 0, (what, x["rc"], x["msg"], y["rc"], y["msg"])
        assert x["pad"] and y["pad"], (what, "a column from B on was written")
        n, bad = E.differing_words(x, y)
        assert n > 0 and bad == 0, (what, n, bad)
        words += n
    return words


@pytest.mark.parametrize("family", list(E.FAMILIES))
def test_leading_dimensions(pkg, dev, fast, fleet, family):
    """ld = B + 3 and ld_warm = B + 2, NaN in the inputs' padding and a sentinel in the outputs': bitwise the call at ld = B, the
    padding untouched.  Device forms: B = 5 on a default handle (the wave kernels, the whole wave per instance) and B = 70 with
    wave_max_batch = -1 (the lane kernel: a full wavefront and a partial one); host forms and the wire form: B = 3.  The rollouts:
    steps = 3, with and without hist."""
    shapes = [(5, fast), (70, E.with_params(fast, wave_max_batch=-1))] if family in E.DEVICE else [(3, fast)]
    for B, params in shapes:
        d = fleet(B)
        with pkg.BatchedMPC(params, B, device=0) as mpc:
            for form in E.forms_of(family):
                for hist in ((True, False) if family in E.ROLLOUT else (True,)):
                    tight = E.sequence(pkg, mpc, dev, family, form, d, hist=hist)
                    loose = E.sequence(pkg, mpc, dev, family, form, d, hist=hist, ld=B + 3, ld_warm=B + 2)
                    words = _same(tight, loose, (family + form, B, hist))
                    print("%s%s B = %d%s: %d words, ld = B + 3 bitwise ld = B" % (family, form, B, "" if hist else " (no hist)", words))


@pytest.mark.parametrize("family", list(E.FAMILIES))
def test_a_null_model_is_the_form_without_model(pkg, dev, fast, fleet, family):
    """_model(model = NULL) is bitwise the plain form and _warm_model(model = NULL) bitwise _warm, the warm buffer written
    included (B = 5)."""
    B = 5
    d = fleet(B)
    with pkg.BatchedMPC(fast, B, device=0) as mpc:
        for form in E.forms_of(family)[1::2]:
            without = E.sequence(pkg, mpc, dev, family, form.replace("_model", ""), d)
            null = E.sequence(pkg, mpc, dev, family, form, d, null_model=True)
            _same(without, null, family + form)
            assert ("warm_out" in null[0]) == ("_warm" in form and family not in E.ROLLOUT)


@pytest.mark.parametrize("handle", list(E.HANDLES))
def test_refusals(pkg, dev, fast, fleet, handle):
    """Every row of the table: the code and the text, on every form the row applies to (B = 16 on a handle with max_batch = 16).  Then
    one good solve on the handle: bitwise a fresh handle's."""
    d = fleet(E.B16)
    params = E.with_params(fast, **E.HANDLES[handle])
    plain = ("mpc_solve_batch_device", "")
    with pkg.BatchedMPC(params, E.B16, device=0) as mpc:
        got = E.refusal_calls(pkg, mpc, dev, d, handle)
        assert len(got) >= 8
        for label, rc, text, want_rc, want_text in got:
            print(label, "->", rc, text)
            assert rc == want_rc and want_text in text, (label, rc, text, want_rc, want_text)
        if handle == "f32":
            return                       # (its good solve takes floats: tests/test_f32.py)
        after = E.call(pkg, mpc, dev, plain[0], plain[1], d)
    with pkg.BatchedMPC(params, E.B16, device=0) as fresh:
        first = E.call(pkg, fresh, dev, plain[0], plain[1], d)
    _same([first], [after], "a good solve after the refusals, " + handle)


def test_cold_fused_model_call_with_max_soc_is_the_stepwise_loop(pkg, dev, fast, fleet):
    d = fleet(E.B16)
    with pkg.BatchedMPC(E.with_params(fast, max_soc=4), E.B16, device=0) as mpc:
        before = mpc.rollout_fused_info()
        r = E.call(pkg, mpc, dev, "mpc_rollout_batch_device_fused", "_model", d, warm_start=0)
        assert r["rc"] == 0, r["msg"]
        after = mpc.rollout_fused_info()
    assert after["stepwise_loops"] == before["stepwise_loops"] + 1 and after["fused_launches"] == before["fused_launches"]


def test_an_empty_batch_with_null_arrays(pkg, dev, fast):
    """B = 0 and NULL arrays: rc 0 from every form.  The device solve forms count the call (mpc_last_batch_id moves by one); every
    other form returns before the solve."""
    with pkg.BatchedMPC(fast, E.B16, device=0) as mpc:
        for family in E.FAMILIES:
            for form in E.forms_of(family):
                before = mpc.last_batch_id()
                rc, text = E.empty_call(pkg, mpc, family, form)
                assert rc == 0, (family + form, rc, text)
                assert mpc.last_batch_id() - before == (1 if family == "mpc_solve_batch_device" else 0), family + form
