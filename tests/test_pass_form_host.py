"""The two form decisions as a plain host program under AddressSanitizer + UndefinedBehaviorSanitizer: `make asan_form` builds
tests/form_harness.cpp, which includes the two HIP-free headers and nothing else of the product.

Which kernels serve a pass of a pool (csrc/aidax_pass_form.h: resolve_pass — the one function behind aidax_pool::launch,
aidax_pool_kernel_name and the blocking path's in-place question): a literal table of rows (facts -> kernel, chains around, end markers,
pieces, in place, name), each restating what the three hand-written copies of the decision did, and properties over the product of the 18
table cells, every forced form, the three modes, eight block lengths, seven pool sizes on 64 and 256 CUs, one to three inputs and the bank
on and off.

Which kind of slot and which SlotForm a model gets at load (csrc/aidax_load_form.h: load_kind, conv_family / conv_form, mfma_form, over the
one-layer rule — what choose_form calls): literal rows (facts -> kind; SlotForm fields, lp, ls, ring_streams; the conv refusal), one at least
for every arm of the choose_form they restate and for every hook value, and properties (ls implies lp; ring_streams is n_streams unless the
form has round_streams; a forced Valu never yields a matrix-core kind; ...) over every hook value, every forced form, six pool sizes, four
block lengths, 8 / 64 / 256 CUs, twelve cells in one to three layers and every answer the kernels' serves / LDS questions can give.
CPU suite only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_pass_form_decision_rows_and_properties_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", ROOT, "asan_form"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "asan", "form_harness")], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "checks, 0 failures" in r.stdout, r.stdout[-3000:]
    n_rows = int(r.stdout.split("form_harness:")[1].split("rows")[0])
    n_checks = int(r.stdout.split("rows,")[1].split("checks")[0])
    assert n_rows >= 80 and n_checks >= 1000000, r.stdout      # one row at least per kernel family and per carried-over behaviour; the whole product
    load = r.stdout.split("(load form:")[1]
    assert int(load.split("rows")[0]) >= 140 and int(load.split("rows,")[1].split("checks")[0]) >= 50000000, r.stdout
