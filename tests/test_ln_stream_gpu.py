"""ln_fwd_kernel reads its rows by the static row count and waits for a packed job's live count only in front of the stores;
ln_bwd_kernel's rows, partials and live-count handling are pinned the same way.

Exact comparisons only.  A row is computed the same way whatever launch it is part of, so the reference of every row is a ONE-ROW
launch of the same kernel on that row, computed once per (D, type) and shared.  What the address change can break is checked
directly: rows at and past the live count keep a sentinel bit pattern, the live count of a prepared job changes on the device between
two launches, and the column partials of a packed launch equal those of a launch whose static row count is the live count.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F16, BF16, I32, I16 = torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.int16
DTYPES = pytest.mark.parametrize("T16", [F16, BF16], ids=["fp16", "bf16"])
SENT16, SENT32 = 0x7BAD, -7777.0
FWD_DS = (8, 96, 520, 768, 1032, 4096)
BWD_DS = (8, 96, 520, 768, 1032, 2048)
# around one wave's walk (2 rows) and one workgroup's rows (8) of the forward; 7 / 16 / 17 are the kernel's own edges
FWD_ROWS = (1, 2, 3, 7, 8, 9, 16, 17, 33, 70)
R = 70
EPS = 1e-6
BWD_WAVES = 8 if os.environ.get("MEMEHIP_LN_BWD_WAVES") == "8" else 4      # rows per workgroup step of ln_bwd_kernel


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import multimodal_propaganda_meme_classification_amd as m
    return m


def _lib(pkg, T16):
    return pkg._lib.load("fp16" if T16 == F16 else "bf16")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sent16(shape, T16):
    return torch.full(shape, SENT16, dtype=I16, device="cuda").view(T16)


def _sent32(shape):
    return torch.full(shape, SENT32, dtype=F32, device="cuda")


def _bits(t):
    return t.view(I16) if t.element_size() == 2 else t.view(I32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sent_mask(t):
    return _bits(t) == (SENT16 if t.element_size() == 2 else _bits(torch.tensor([SENT32]))[0].item())


def _is_sent(t):
    return bool(_sent_mask(t).all())


def _dev_int(n):
    return torch.tensor([n], dtype=I32, device="cuda")


def _inputs(D, T16, rows=R, seed=0):
    g = torch.Generator().manual_seed(77 * D + seed)
    x = (torch.randn(rows, D, generator=g) * 1.5 + 0.25).to(T16).cuda()
    dy = (torch.randn(rows, D, generator=g) * 0.5).to(T16).cuda()
    add = torch.randn(rows, D, generator=g).to(T16).cuda()
    gamma = (1.0 + 0.2 * torch.randn(D, generator=g)).cuda()
    beta = (0.3 * torch.randn(D, generator=g)).cuda()
    return x, dy, add, gamma, beta


# ------------------------------------------------------------------------------------------------------------------ forward

def _fwd_outputs(rows, D, T16):
    return dict(y=_sent16((rows, D), T16), y32=_sent32((rows, D)), mean=_sent32((rows,)), rstd=_sent32((rows,)))


def _fwd_fill(pkg, jobs):
    arr = (pkg._lib.MhLnFwdJob * len(jobs))()
    for e, j in zip(arr, jobs):
        e.x, e.gamma, e.beta, e.y, e.y_f32 = _ptr(j["x"]), _ptr(j["gamma"]), _ptr(j["beta"]), _ptr(j["y"]), _ptr(j["y32"])
        e.mean, e.rstd, e.rows, e.eps, e.rows_dev = _ptr(j["mean"]), _ptr(j["rstd"]), j["rows"], EPS, _ptr(j.get("rows_dev"))
    return arr


def _fwd_go(pkg, T16, D, arr):
    pkg._lib.check(_lib(pkg, T16).mh_layernorm_fwd_grouped(arr, len(arr), D, _st()), "mh_layernorm_fwd_grouped")


_FWD_REF = {}


def _fwd_ref(pkg, D, T16):
    """(inputs, outputs of R one-row launches), once per (D, type)"""
    key = (D, T16)
    if key not in _FWD_REF:
        x, dy, add, gamma, beta = _inputs(D, T16)
        out = _fwd_outputs(R, D, T16)
        for r in range(R):
            _fwd_go(pkg, T16, D, _fwd_fill(pkg, [dict(x=x[r:r + 1], gamma=gamma, beta=beta, rows=1, **{k: t[r:r + 1] for k, t in out.items()})]))
        torch.cuda.synchronize()
        assert not any(bool(_sent_mask(t).any()) for t in out.values())
        _FWD_REF[key] = ((x, gamma, beta), out)
    return _FWD_REF[key]


@DTYPES
@pytest.mark.parametrize("D", FWD_DS, ids=[f"D{d}" for d in FWD_DS])
def test_ln_forward_partition_independence(pkg, D, T16):
    (x, gamma, beta), ref = _fwd_ref(pkg, D, T16)
    for rows in FWD_ROWS:
        out = _fwd_outputs(R, D, T16)
        _fwd_go(pkg, T16, D, _fwd_fill(pkg, [dict(x=x, gamma=gamma, beta=beta, rows=rows, **out)]))
        torch.cuda.synchronize()
        for k in out:
            assert _same(out[k][:rows], ref[k][:rows]), f"D={D} rows={rows}: {k} differs from the one-row launches"
            assert _is_sent(out[k][rows:]), f"D={D} rows={rows}: {k} written past the launch's rows"


@DTYPES
@pytest.mark.parametrize("D", (96, 768, 1032), ids=lambda d: f"D{d}")
def test_ln_forward_grouped_live_counts(pkg, D, T16):
    (x, gamma, beta), ref = _fwd_ref(pkg, D, T16)
    specs = [(70, 0), (33, 20), (9, 9), (17, 3)]             # (rows the buffers hold, live rows on the device)
    jobs = [dict(x=x[:rows], gamma=gamma, beta=beta, rows=rows, rows_dev=_dev_int(live), **_fwd_outputs(rows, D, T16)) for rows, live in specs]
    arr = _fwd_fill(pkg, jobs)

    def check(lives, tag):
        torch.cuda.synchronize()
        for j, live in zip(jobs, lives):
            for k in ("y", "y32", "mean", "rstd"):
                assert _same(j[k][:live], ref[k][:live]), f"{tag} D={D} rows={j['rows']} live={live}: {k} differs from the one-row launches"
                assert _is_sent(j[k][live:]), f"{tag} D={D} rows={j['rows']} live={live}: {k} written at or past the live count"

    _fwd_go(pkg, T16, D, arr)
    check([live for _, live in specs], "first")
    # the packed text tower's use: the SAME prepared jobs, the live counts changed on the device between two launches
    for lives in ([1, 33, 0, 17], [70, 7, 8, 0]):
        for j, live in zip(jobs, lives):
            j["rows_dev"].fill_(live)
            j["y"].view(I16).fill_(SENT16)
            for k in ("y32", "mean", "rstd"):
                j[k].fill_(SENT32)
        _fwd_go(pkg, T16, D, arr)
        check(lives, f"relaunch {lives}")


# ----------------------------------------------------------------------------------------------------------------- backward

def _rng(seed=4321, step=3):
    return torch.tensor([seed & 0x7FFFFFFF, (seed >> 31) & 0x7FFFFFFF, step, 0], dtype=I32, device="cuda")


def _bwd_fill(pkg, jobs):
    arr = (pkg._lib.MhLnBwdJob * len(jobs))()
    for e, j in zip(arr, jobs):
        e.dy, e.x, e.gamma, e.mean, e.rstd = _ptr(j["dy"]), _ptr(j["x"]), _ptr(j["gamma"]), _ptr(j["mean"]), _ptr(j["rstd"])
        e.dx_add, e.dx, e.part, e.dx_drop = _ptr(j.get("dx_add")), _ptr(j["dx"]), _ptr(j["part"]), _ptr(j.get("dx_drop"))
        drop = j.get("dx_drop") is not None
        e.rng, e.drop_p, e.drop_stream = (_ptr(j["rng"]), 0.1, 31) if drop else (None, 0.0, 0)
        e.n_part, e.rows = j["n_part"], j["rows"]
        e.rows_dev, e.drop_rows = _ptr(j.get("rows_dev")), _ptr(j.get("drop_rows"))
    return arr


def _bwd_go(pkg, T16, D, arr):
    pkg._lib.check(_lib(pkg, T16).mh_layernorm_bwd_grouped(arr, len(arr), D, _st()), "mh_layernorm_bwd_grouped")


VARIANTS = ("plain", "add", "drop")
_BWD_REF = {}


def _bwd_job(variant, ins, rows, n_part, D, T16, lo=0, out=None, **kw):
    """a job over rows [lo, lo + rows) of the shared inputs; outputs allocated sentinel-filled unless given"""
    x, dy, add, gamma, mean, rstd, drop_rows, rng = ins
    sl = slice(lo, lo + rows)
    j = dict(dy=dy[sl], x=x[sl], gamma=gamma, mean=mean[sl], rstd=rstd[sl], rows=rows, n_part=n_part, **kw)
    j["dx"] = _sent16((rows, D), T16) if out is None else out["dx"][sl]
    j["part"] = _sent32((2, n_part, D))
    if variant == "add":
        j["dx_add"] = add[sl]
    if variant == "drop":
        j["dx_drop"] = _sent16((rows, D), T16) if out is None else out["dx_drop"][sl]
        j["drop_rows"], j["rng"] = drop_rows[sl], rng
    return j


def _bwd_ref(pkg, D, T16):
    """(inputs, {variant: dx / dx_drop of R one-row launches}), once per (D, type)"""
    key = (D, T16)
    if key not in _BWD_REF:
        x, dy, add, gamma, beta = _inputs(D, T16, seed=1)
        mean, rstd = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
        y = torch.empty_like(x)
        _fwd_go(pkg, T16, D, _fwd_fill(pkg, [dict(x=x, gamma=gamma, beta=beta, rows=R, y=y, y32=None, mean=mean, rstd=rstd)]))
        drop_rows = (torch.randperm(R, generator=torch.Generator().manual_seed(D)) * 3 + 5).to(I32).cuda()     # mask rows of the packed layout
        ins = (x, dy, add, gamma, mean, rstd, drop_rows, _rng())
        refs = {}
        for variant in VARIANTS:
            out = dict(dx=_sent16((R, D), T16), dx_drop=_sent16((R, D), T16))
            for r in range(R):
                _bwd_go(pkg, T16, D, _bwd_fill(pkg, [_bwd_job(variant, ins, 1, 1, D, T16, lo=r, out=out)]))
            torch.cuda.synchronize()
            assert not bool(_sent_mask(out["dx"]).any()) and (variant != "drop" or not bool(_sent_mask(out["dx_drop"]).any()))
            refs[variant] = out
        _BWD_REF[key] = (ins, refs)
    return _BWD_REF[key]


def _check_bwd(tag, j, ref, live, n_part):
    for k in ("dx", "dx_drop"):
        if j.get(k) is None:
            continue
        assert _same(j[k][:live], ref[k][:live]), f"{tag}: {k} differs from the one-row launches"
        assert _is_sent(j[k][live:]), f"{tag}: {k} written at or past the live count"
    assert not bool(_sent_mask(j["part"]).any()) and bool(torch.isfinite(j["part"]).all()), f"{tag}: a partial row was not written"
    first_dead = -(-live // BWD_WAVES)          # workgroup b owns rows b * waves + w (+ k * n_part * waves): none is live from here on
    if first_dead < n_part:
        assert bool((_bits(j["part"][:, first_dead:]) == 0).all()), f"{tag}: the partials of a workgroup without a live row are not +0"


@DTYPES
@pytest.mark.parametrize("D", BWD_DS, ids=[f"D{d}" for d in BWD_DS])
def test_ln_backward_partition_independence(pkg, D, T16):
    ins, refs = _bwd_ref(pkg, D, T16)
    for variant in VARIANTS:
        for n_part in (1, 3, 8, 64):
            for rows in (1, 9, 33, R):
                j = _bwd_job(variant, ins, rows, n_part, D, T16)
                _bwd_go(pkg, T16, D, _bwd_fill(pkg, [j]))
                torch.cuda.synchronize()
                _check_bwd(f"{variant} D={D} n_part={n_part} rows={rows}", j, refs[variant], rows, n_part)


@DTYPES
@pytest.mark.parametrize("D", (96, 768, 1032), ids=lambda d: f"D{d}")
def test_ln_backward_live_counts(pkg, D, T16):
    ins, refs = _bwd_ref(pkg, D, T16)
    for variant in VARIANTS:
        for n_part in (1, 3, 8, 64):
            static = {}
            for live in (0, 1, 37, R):
                if live:                      # what a launch sized for the live rows alone leaves in the partials
                    s = _bwd_job(variant, ins, live, n_part, D, T16)
                    _bwd_go(pkg, T16, D, _bwd_fill(pkg, [s]))
                    static[live] = s["part"]
                else:
                    static[live] = torch.zeros((2, n_part, D), device="cuda")
            j = _bwd_job(variant, ins, R, n_part, D, T16, rows_dev=_dev_int(0))
            arr = _bwd_fill(pkg, [j])
            for live in (37, 0, R, 1, 37):    # the same prepared job, the live count changed on the device between launches
                j["rows_dev"].fill_(live)
                for k in ("dx", "dx_drop"):
                    if j.get(k) is not None:
                        j[k].view(I16).fill_(SENT16)
                j["part"].fill_(SENT32)
                _bwd_go(pkg, T16, D, arr)
                torch.cuda.synchronize()
                tag = f"{variant} D={D} n_part={n_part} live={live}"
                _check_bwd(tag, j, refs[variant], live, n_part)
                assert _same(j["part"], static[live]), f"{tag}: partials differ from a launch sized for the live rows"


@DTYPES
def test_ln_backward_grouped_jobs(pkg, T16):
    D = 768
    ins, refs = _bwd_ref(pkg, D, T16)
    specs = [("plain", 70, None, 8), ("drop", 33, 20, 3), ("add", 9, 9, 64), ("drop", 17, 0, 1)]      # (variant, rows, live, n_part)
    jobs = [_bwd_job(v, ins, rows, n_part, D, T16, **({} if live is None else dict(rows_dev=_dev_int(live)))) for v, rows, live, n_part in specs]
    _bwd_go(pkg, T16, D, _bwd_fill(pkg, jobs))
    torch.cuda.synchronize()
    for j, (v, rows, live, n_part) in zip(jobs, specs):
        _check_bwd(f"grouped {v} rows={rows} live={live}", j, refs[v], rows if live is None else live, n_part)
