"""Classification routing on the host (no GPU, no launch): which kernels `ops.classify` takes is a function of the call — shape, wanted outputs, alpha and the
routing context managers of the calling context — and of nothing global.  The route table was recorded from the library before routing moved into per-call flags."""
import ctypes
import threading
from contextlib import ExitStack

import pytest

from proto_clip_amd import _lib, ops

# context-manager stacks, in the column order of ROUTES
CONTEXTS = (
    (),
    (lambda: ops.classify_mid(0),),
    (lambda: ops.classify_mid(2),),
    (ops.classify_two_stage,),
    (ops.classify_fused,),
    (ops.classify_fused, lambda: ops.classify_mid(2)),
    (ops.classify_two_stage, lambda: ops.classify_mid(2)),
    (ops.classify_fused, lambda: ops.classify_panel_passes(1), ops.classify_panel_exact),
)
# wanted outputs, one group of ROUTES digits each
WANTS = (dict(), dict(want_p=True, want_argmax=False), dict(want_p=True), dict(topk=5), dict(has_zt=False))
# (Q, N, D, alpha): for each of WANTS, the route (index into ops.CLASSIFY_ROUTES) under each of CONTEXTS; beta = 12
ROUTES = {
    (8100, 10, 512, 0.5): '11211221 11211221 11211221 11111111 11111111',
    (300, 17, 512, 0.5): '21211221 21211221 21211221 11111111 11111111',
    (4000, 32, 512, 0.5): '21211221 21211221 21211221 11111111 11111111',
    (300, 37, 512, 0.5): '20203223 20200220 20200220 00000000 00000000',
    (2465, 100, 1024, 0.5): '20203223 20200220 20200220 00000000 00000000',
    (666, 198, 768, 0.5): '20203223 20200220 20200220 00000000 00000000',
    (300, 256, 1024, 0.5): '20203223 20200220 20200220 00000000 00000000',
    (15000, 198, 768, 0.5): '00203223 00200220 00200220 00000000 00000000',
    (300, 100, 576, 0.5): '00003303 00000000 00000000 00000000 00000000',
    (1, 37, 768, 0.5): '20203223 20200220 20200220 00000000 00000000',
    (1024, 1000, 512, 0.5): '00003303 00000000 00000000 00000000 00000000',
    (50000, 1000, 512, 0.5): '33303303 00000000 00000000 00000000 00000000',
    (50000, 1000, 512, 1.2): '00000000 00000000 00000000 00000000 00000000',
    (600, 4096, 4096, 0.5): '00003303 00000000 00000000 00000000 00000000',
    (20000, 4096, 512, 0.5): '33303303 00000000 00000000 00000000 00000000',
    (15000, 256, 768, 0.5): '33203223 00200220 00200220 00000000 00000000',
}


def routes_of(Q, N, D, alpha):
    groups = []
    for kw in WANTS:
        digits = ""
        for makers in CONTEXTS:
            with ExitStack() as stack:
                for make in makers:
                    stack.enter_context(make())
                digits += str(ops.CLASSIFY_ROUTES.index(ops.classify_route(Q, N, D, alpha, 12.0, **kw)))
        groups.append(digits)
    return " ".join(groups)


@pytest.mark.parametrize("shape", list(ROUTES))
def test_route_table(shape):
    assert routes_of(*shape) == ROUTES[shape]


def test_no_small_flag():
    lib = _lib.load()
    ws = _lib.workspace_bytes(_lib.OP_CLASSIFY, 8100, 10, 512)
    assert lib.pclip_classify_route_ex(8100, 10, 512, 0.5, 0.5, 12.0, 1, 0, 1, 0, 0, ws) == 1
    assert lib.pclip_classify_route_ex(8100, 10, 512, 0.5, 0.5, 12.0, 1, 0, 1, 0, _lib.CLASSIFY_NO_SMALL, ws) == 0
    assert lib.pclip_classify_route(8100, 10, 512, 0.5, 0.5, 12.0, 1, 0, 1, 0, ws) == 1


def test_threads_route_by_their_own_context():
    """Two threads inside different context managers at the same time get their own routes for the same shape."""
    Q, N, D = 2465, 100, 1024
    barrier = threading.Barrier(2, timeout=30)
    got = {}

    def run(name, cm):
        with cm():
            barrier.wait()                                  # both contexts are entered before either thread asks
            first = ops.classify_route(Q, N, D, 0.5, 12.0)
            barrier.wait()
            got[name] = (first, ops.classify_route(Q, N, D, 0.5, 12.0))

    threads = [threading.Thread(target=run, args=("two", ops.classify_two_stage)), threading.Thread(target=run, args=("mid", lambda: ops.classify_mid(2)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got == {"two": ("two stages",) * 2, "mid": ("one launch, mid N",) * 2}
    assert ops.classify_route(Q, N, D, 0.5, 12.0) == "one launch, mid N"


@pytest.mark.parametrize("Q,N,D", [(300, 1000, 512), (600, 4096, 4096), (50000, 1000, 512), (2465, 100, 1024), (8100, 10, 512)])
def test_workspace_is_a_function_of_the_shape(Q, N, D):
    before = _lib.workspace_bytes(_lib.OP_CLASSIFY, Q, N, D)
    for cm in (ops.classify_two_stage, ops.classify_fused, lambda: ops.classify_mid(2), ops.classify_panel_exact):
        with cm():
            assert _lib.workspace_bytes(_lib.OP_CLASSIFY, Q, N, D) == before
        assert _lib.workspace_bytes(_lib.OP_CLASSIFY, Q, N, D) == before


@pytest.mark.parametrize("flags", [0x100, -1, _lib.CLASSIFY_NO_MID | _lib.CLASSIFY_FORCE_MID, _lib.CLASSIFY_NO_PANELS | _lib.CLASSIFY_FORCE_PANELS,
                                   _lib.CLASSIFY_PANEL_TWO_PASS | _lib.CLASSIFY_PANEL_FORCE_SECOND])
def test_invalid_flags_are_refused(flags):
    lib = _lib.load()
    buf = ctypes.c_void_p(0x1000)      # never dereferenced: validation rejects first
    assert lib.pclip_classify_route_ex(300, 100, 512, 0.5, 0.5, 12.0, 1, 0, 1, 0, flags, 1 << 30) == -1
    assert b"flags" in lib.pclip_last_error()
    assert lib.pclip_classify_ex_f16(buf, buf, buf, 0, 100, 512, None, None, None, 0.5, 0.5, 12.0, None, buf, None, None, 0, flags, buf, 1 << 30, None) == -1
    assert b"flags" in lib.pclip_last_error()
    valid = _lib.CLASSIFY_NO_SMALL | _lib.CLASSIFY_NO_MID | _lib.CLASSIFY_FORCE_PANELS | _lib.CLASSIFY_PANEL_FORCE_SECOND | _lib.CLASSIFY_PANEL_EXACT
    assert lib.pclip_classify_ex_f16(buf, buf, buf, 0, 100, 512, None, None, None, 0.5, 0.5, 12.0, None, buf, None, None, 0, valid, buf, 1 << 30, None) == 0
