"""The one-layer rule (csrc/aidax_load_form.h: many_streams_form, with lone_split_pays and lstm_gs_pays inside it) against the commit before
it became pure functions of (cell, hidden, streams, CUs, block length, FormHooks), over the whole domain. No GPU.

tests/golden/many_streams_parent.json holds, per (cell, hidden, CUs, block length, hooks), the CHANGE POINTS of aidax_many_streams_form_at
along GRID's stream counts: [n, form] for the first count and for every count whose form differs from the count before it. It was recorded
ONCE from the test-hooks library of the parent commit (65d3f83), through the binding:
    AIDAX_LIB=<that commit's aidadsp-lv2_amd/lib/hooks/libaidax_hip.so> python -m tests.test_many_streams_host --record <out.json>
(the __main__ block at the end of this file; the same _change_points as the test). Equal change points over the same grid are equal forms
at every point of it; no point is excluded.

  cells          the 18 of the kernel table, (LSTM, 48) and (GRU, 96) (no table kernel), and an unknown cell id
  CUs            0 (unknown: taken for 256), 32, 64, 256, 304
  block lengths  4, 63, 64, 191, 192, 256
  stream counts  every n within one of a multiple of 16 up to five rounds of stream groups (80 x CUs streams); on 32 CUs every n
  hooks          at 256 CUs and blocks of 64 and 256 frames: AIDAX_LSTM_GS {unset, 0, 1} x AIDAX_LS1 {unset, 0} x AIDAX_LP_SPLIT {unset, 0} x
                 AIDAX_GRU_GM {unset, f32, 0}
"""
import importlib
import itertools
import json
import os
import sys

ax = importlib.import_module("aidadsp-lv2_amd")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "many_streams_parent.json")
PARENT = "65d3f83"
CELLS = [(c, h) for c in (0, 1) for h in (8, 12, 16, 20, 24, 32, 40, 64, 80)] + [(0, 48), (1, 96), (7, 32)]
CUS = (0, 32, 64, 256, 304)
FRAMES = (4, 63, 64, 191, 192, 256)
HOOKS = ("AIDAX_LSTM_GS", "AIDAX_LS1", "AIDAX_LP_SPLIT", "AIDAX_GRU_GM")
HOOK_SETS = [dict((k, v) for k, v in zip(HOOKS, vals) if v is not None)
             for vals in itertools.product((None, "0", "1"), (None, "0"), (None, "0"), (None, "f32", "0"))]


def _grid(cus):
    rounds = 5 * (cus if cus > 0 else 256)                  # stream groups of five rounds
    if cus == 32:
        return range(1, 16 * rounds + 2)
    return [n for k in range(rounds + 1) for n in (16 * k - 1, 16 * k, 16 * k + 1) if n >= 1]


def _change_points(cell, hidden, cus, frames):
    f = ax.lib().aidax_many_streams_form_at
    out, prev = [], None
    for n in _grid(cus):
        v = f(cell, hidden, n, cus, frames)
        if v != prev:
            out.append([n, v])
            prev = v
    return out


def _key(cell, hidden, cus, frames, hooks):
    return f"{cell} {hidden} {cus} {frames} " + (",".join(f"{k[6:]}={v}" for k, v in sorted(hooks.items())) or "-")


def _cases():
    """(key, hooks, arguments) of every line of the fixture: the plain domain, then the hook product"""
    for cell, hidden in CELLS:
        for cus in CUS:
            for frames in FRAMES:
                yield _key(cell, hidden, cus, frames, {}), {}, (cell, hidden, cus, frames)
    for hooks in HOOK_SETS:
        if not hooks:
            continue
        for cell, hidden in CELLS:
            for frames in (64, 256):
                yield _key(cell, hidden, 256, frames, hooks), hooks, (cell, hidden, 256, frames)


def _all_points(setenv, delenv):
    got, at = {}, None
    for key, hooks, args in _cases():
        if hooks != at:
            for k in HOOKS:
                delenv(k)
            for k, v in hooks.items():
                setenv(k, v)
            at = hooks
        got[key] = _change_points(*args)
    for k in HOOKS:
        delenv(k)
    return got


def test_the_one_layer_rule_equals_the_parent_commits_over_the_whole_domain(monkeypatch):
    with open(FIXTURE) as f:
        fixture = json.load(f)
    assert fixture["parent"] == PARENT
    want = fixture["change_points"]
    got = _all_points(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert len(got) == len(CELLS) * len(CUS) * len(FRAMES) + (len(HOOK_SETS) - 1) * len(CELLS) * 2 == 630 + 35 * 21 * 2
    assert sorted(got) == sorted(want)                         # the fixture has every line of the domain and no other
    bad = [k for k in got if got[k] != want[k]]
    for k in bad[:10]:
        print(f"{k}: got {got[k]}\n{' ' * len(k)}  want {want[k]}")
    assert not bad, f"{len(bad)} of {len(got)} lines differ from the parent commit"
    # the grid is the one the docstring states: the hooked and the 256-CU lines probe 3 x 1281 - 2 counts, a 32-CU line every count up to 2561
    assert len(_grid(256)) == 3 * 1281 - 2 and len(_grid(0)) == len(_grid(256)) and list(_grid(32)) == list(range(1, 2562)) and _grid(304)[-1] == 24321


if __name__ == "__main__":
    # records a fixture from whatever library AIDAX_LIB names (see the module docstring); the path is required, and the committed fixture is
    # never written over: it is the parent commit's, recorded once
    if "--record" in sys.argv:
        k = sys.argv.index("--record")
        if len(sys.argv) <= k + 1 or os.path.abspath(sys.argv[k + 1]) == FIXTURE:
            raise SystemExit("usage: python -m tests.test_many_streams_host --record <out.json>  (not the committed fixture)")
        points = _all_points(os.environ.__setitem__, lambda k_: os.environ.pop(k_, None))
        with open(sys.argv[k + 1], "w") as f:
            json.dump({"parent": PARENT, "function": "aidax_many_streams_form_at", "change_points": points}, f, separators=(",", ":"))
        print(f"recorded {len(points)} lines from {ax.lib_path()} -> {sys.argv[k + 1]} ({os.path.getsize(sys.argv[k + 1])} bytes)")
