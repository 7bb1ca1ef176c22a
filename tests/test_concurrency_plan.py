"""CPU (no device needed): the host side of the library from several threads at once.  include/dau_conv.h calls dau_conv_last_error
a "thread-local message of the last failing call" and lets a cached plan be shared by threads; plan creation runs
the cost models, the variant tables and the function-local statics of the library, none of which another test enters from two threads.

Eight threads behind a barrier create, 50 times over, a plan of each of a dozen descriptors -- the three plan families of
test_gpu_concurrency.py, the layer of test_gpu_concurrency_layer.py and a few of test_line_dot_plan.py's -- read everything a plan
answers without a device, and drop it.  Every answer must be the one the main thread got for that descriptor before the threads
started.  Between the plans every thread asks for an invalid flag pair of its own: two pairs with different messages, and each
thread must find the message of ITS refusal in the exception."""
import threading

import pytest

THREADS, ROUNDS, JOIN_SECONDS = 8, 50, 120


def _descriptors():
    from dau_conv import _capi as c
    I, SD = c.FLAG_USE_INTERPOLATION, c.FLAG_SINGLE_DIM_KERNEL
    line = I | SD | c.FLAG_DENSE_SPLIT_F16 | c.FLAG_DENSE_SPLIT_LINE | c.FLAG_SPLIT_DOT_LINE
    return [
        # the plan families of test_gpu_concurrency.py
        dict(shape=(2, 6, 24, 4, 28, 28), k=17, flags=I | c.FLAG_DENSE_SPLIT_F16),
        dict(shape=(3, 5, 9, 3, 13, 21), k=33, flags=I | c.FLAG_NO_DENSE_SPLIT | c.FLAG_IO_F16 | c.FLAG_IO_NHWC),
        dict(shape=(9, 7, 5, 2, 9, 6), k=17, flags=line),
        dict(shape=(2, 6, 24, 4, 28, 28), k=9, flags=I | c.FLAG_DENSE_SPLIT_F16),
        # the layers of test_gpu_concurrency_layer.py
        dict(shape=(4, 12, 24, 4, 28, 28), k=9, flags=I),
        dict(shape=(4, 48, 48, 4, 56, 56), k=9, flags=I),
        # of test_line_dot_plan.py: forced and default plans with the gather-dot's line members, 16-bit and NHWC forms
        dict(shape=(2, 16, 16, 2, 16, 16), k=11, flags=I | SD | c.FLAG_DENSE_SPLIT_F16 | c.FLAG_SPLIT_DOT_LINE),
        dict(shape=(2, 32, 32, 3, 20, 20), k=17, flags=I | SD | c.FLAG_SPLIT_DOT_LINE),
        dict(shape=(2, 32, 32, 5, 20, 20), k=17, flags=I | SD | c.FLAG_SPLIT_DOT_LINE),
        dict(shape=(2, 7, 5, 4, 16, 16), k=17, flags=line | c.FLAG_IO_BF16 | c.FLAG_IO_NHWC | c.FLAG_INPUT_RELU),
        # a wide layer (every two-limb member by default), and one on the direct kernels
        dict(shape=(2, 128, 128, 4, 16, 16), k=9, flags=I),
        dict(shape=(2, 3, 4, 2, 8, 9), k=9, flags=I, algo=1),
    ]


def _refusals():
    from dau_conv import _capi as c
    I = c.FLAG_USE_INTERPOLATION
    return [(I | c.FLAG_DENSE_SPLIT_LINE, "DAU_FLAG_DENSE_SPLIT_LINE needs DAU_FLAG_SINGLE_DIM_KERNEL"),
            (I | c.FLAG_DENSE_SPLIT_OUTLIERS | c.FLAG_NO_DENSE_SPLIT, "DAU_FLAG_DENSE_SPLIT_OUTLIERS excludes")]


def _answers(d):
    """everything a plan answers without a device, as one comparable value"""
    from dau_conv import _capi as c
    plan = c.Plan(*d["shape"], max_kernel_size=d["k"], flags=d["flags"], algo=d.get("algo", 0), sigma_hint=0.5)
    sizes = []
    for which in (c.PASS_FORWARD, c.PASS_BACKWARD, c.PASS_EPILOGUE_BACKWARD):
        try:
            sizes.append(plan.workspace_bytes(which))
        except c.DAUConvError as e:                           # (a pass the plan does not have: the refusal is the answer)
            sizes.append(str(e))
    out = (tuple(sorted(plan.info.items())), tuple(sizes), plan.split_dot_geometry(), plan.last_status(), plan.sigma_status())
    del plan
    return out


def _refused(flags):
    from dau_conv import _capi as c
    try:
        c.Plan(2, 8, 8, 2, 8, 8, flags=flags)
    except c.InvalidArgumentError as e:
        return str(e)
    return "(not refused)"


def test_plans_created_and_asked_from_eight_threads():
    descs, refusals = _descriptors(), _refusals()
    assert len(descs) == 12
    want = [_answers(d) for d in descs]
    assert len(set(want)) == len(want), "the descriptors were meant to give twelve different plans"
    for flags, text in refusals:
        assert text in _refused(flags)
    assert refusals[0][1] not in _refused(refusals[1][0]) and refusals[1][1] not in _refused(refusals[0][0])
    barrier = threading.Barrier(THREADS)
    failures = [None] * THREADS

    def work(t):
        try:
            flags, text = refusals[t % 2]
            barrier.wait(JOIN_SECONDS)
            for rnd in range(ROUNDS):
                for i in range(len(descs)):
                    j = (i + t) % len(descs)                  # every thread starts at another descriptor
                    got = _answers(descs[j])
                    assert got == want[j], "thread %d round %d descriptor %d: %r, single-threaded %r" % (t, rnd, j, got, want[j])
                    if i % 4 == 0:
                        msg = _refused(flags)
                        assert text in msg, "thread %d round %d: asked for flags 0x%x, the exception says %r" % (t, rnd, flags, msg)
        except BaseException as e:                            # noqa: B902 (kept for the main thread, which raises it)
            failures[t] = e

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(JOIN_SECONDS)
    assert not any(th.is_alive() for th in threads), "a thread is still creating plans after %d s" % JOIN_SECONDS
    for e in failures:
        if e is not None:
            raise e


def test_last_error_of_a_thread_that_never_failed_is_empty():
    """dau_conv_last_error is thread-local: a fresh thread reads "" whatever the main thread's last refusal said."""
    from dau_conv import _capi as c
    flags, text = _refusals()[0]
    assert text in _refused(flags) and text.encode() in c.lib.dau_conv_last_error()
    seen = []
    th = threading.Thread(target=lambda: seen.append(c.lib.dau_conv_last_error()), daemon=True)
    th.start()
    th.join(JOIN_SECONDS)
    assert seen == [b""], seen
    assert text.encode() in c.lib.dau_conv_last_error()      # and the main thread's message is still its own
