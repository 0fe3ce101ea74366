"""CPU: gsd_act_once_pays, the host model that decides per tensor whether relu(bn(raw)) is written once (include/gsd.h).  The
query reads no device memory."""
import pytest

DIMS, H0, W0 = [64, 128, 256, 512, 1024], 320, 427


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gelslim_depth_amd import _lib
    return _lib.lib


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("GSD_ACT_ONCE_FORCE", "GSD_CONV_W2D", "GSD_CONV_ALGO", "GSD_W2D_X4", "GSD_W2D_TW", "GSD_W2D_SPLIT"):
        monkeypatch.delenv(k, raising=False)


def flagship():
    """(kind, level, Cact, Cin, Cout, h, w, pass_kind) of the 13 + 4 forward convs that read an activated or pooled tensor."""
    out, h, w = [], H0, W0
    for lvl, c in enumerate(DIMS):
        if lvl:
            out.append(("enc0", lvl, c // 2, c // 2, c, h, w, 2))
        out.append(("mid", lvl, c, c, c, h, w, 0))
        if lvl < 4:
            out.append(("dec0", lvl, c, 2 * c, c, h, w, 1))
            out.append(("mid", lvl, c, c, c, h, w, 0))
        h, w = h // 2, w // 2
    return out


def test_declines_when_the_consumer_is_not_the_2d_form(lib, monkeypatch):
    assert lib.gsd_act_once_pays(32, 80, 106, 256, 256, 256, 0, 0, 0) == 1
    monkeypatch.setenv("GSD_CONV_W2D", "0")                       # every Winograd launch takes the row form
    assert lib.gsd_act_once_pays(32, 80, 106, 256, 256, 256, 0, 0, 0) == 0
    monkeypatch.delenv("GSD_CONV_W2D")
    # the deep levels at batch 8 stay with the row form's K slabs (gsd_conv3x3_prefers_w2d): nothing to save there
    assert lib.gsd_conv3x3_prefers_w2d(8, 20, 26, 1024, 1024, 1) == 0
    assert lib.gsd_act_once_pays(8, 20, 26, 1024, 1024, 1024, 0, 0, 0) == 0
    # 3 input channels: no 2-D form at all; and an override cannot force what the launch does not admit
    monkeypatch.setenv("GSD_ACT_ONCE_FORCE", "1")
    assert lib.gsd_act_once_pays(32, 320, 427, 3, 3, 64, 0, 0, 0) == 0
    assert lib.gsd_act_once_pays(32, 160, 213, 128, 128, 128, 0, 0, 0) == 1       # forced where the model alone declines
    monkeypatch.setenv("GSD_W2D_X4", "0")
    assert lib.gsd_act_once_pays(32, 160, 213, 128, 128, 128, 0, 0, 0) == 0


def test_declines_a_pad_offset(lib):
    assert lib.gsd_act_once_pays(32, 160, 213, 128, 256, 128, 0, 0, 1) == 1
    assert lib.gsd_act_once_pays(32, 160, 213, 128, 256, 128, 0, 1, 1) == 0
    assert lib.gsd_act_once_pays(32, 160, 213, 128, 256, 128, 1, 0, 1) == 0


def test_monotone_in_the_batch(lib):
    """Saving and cost are both linear in the batch and only the cost has a constant part (the launch), so among the batches at
    which the consumer takes the 2-D form a tensor that pays at one batch pays at every larger one."""
    for kind, lvl, ca, ci, co, h, w, pk in flagship():
        seen = False
        for n in (1, 2, 4, 8, 16, 32, 64, 128):
            if not lib.gsd_conv3x3_prefers_w2d(n, h, w, ci, co, 1):
                continue
            pays = bool(lib.gsd_act_once_pays(n, h, w, ca, ci, co, 0, 0, pk))
            assert pays or not seen, (kind, lvl, n)
            seen = seen or pays


def test_flagship_answers_as_the_recorded_fit(lib):
    """Batch 32 at 3 x 320 x 427, the fit recorded in gsd_conv3x3_host.h from profiles/act_once_layers_b32.txt: the pooled tensors
    always (no cost); the stand-alone pass from the 80 x 106 level down (measured: 155 us saved for an 88 us pass there, 112 for 177
    at 160 x 213, 81 for 355 at 320 x 427); the skip tensor from 160 x 213 down (195 for 90; 153 for 178 at 320 x 427)."""
    for kind, lvl, ca, ci, co, h, w, pk in flagship():
        want = {"enc0": 1, "mid": int(lvl >= 2), "dec0": int(lvl >= 1)}[kind]
        assert lib.gsd_act_once_pays(32, h, w, ca, ci, co, 0, 0, pk) == want, (kind, lvl)
    # the cheaper the pass, the sooner it pays
    assert lib.gsd_act_once_pays(32, 160, 213, 128, 128, 128, 0, 0, 0) == 0
    assert lib.gsd_act_once_pays(32, 160, 213, 128, 256, 128, 0, 0, 1) == 1
    assert lib.gsd_act_once_pays(32, 320, 427, 64, 64, 64, 0, 0, 2) == 1
