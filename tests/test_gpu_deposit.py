"""Exact sample deposits on the MI355X (tor_deposit_device, Context.deposit, Film).

The open pipeline -- camera rays, radiance, deposit -- must give tor_render_accumulate_device's sums and moments in every bit,
whatever the order and the split of the entries; synthetic entries must give the bits, counts and rejections of the numpy
restatement (tests/deposit_restatement.py, held to hand-worked cases by tests/test_deposit.py, which also shows that the inputs
of tests/deposit_inputs.py mean something).  What the kernel may break: a run of a wave reduced into the wrong head or flushed
twice (A B A B), a sample lost at a wave or workgroup boundary, a rejected or foreign lane carried into a run, a moment taken
from the unquantised colour, a channel dropped where the whole sample must be."""
import numpy as np
import pytest
import torch

import deposit_inputs as I
import deposit_restatement as D

pytestmark = pytest.mark.gpu
NROWS, NCOLS, DEPTH = 24, 16, 8


def _cuda(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


class Buffers:
    """Device film buffers, zero or copies of a restated result."""

    def __init__(self, npix, into=None, moments=True, counts=True, rejected=True):
        z = D._start(into, npix)
        self.sums = _cuda(z[0])
        self.moments = _cuda(z[1]) if moments else None
        self.counts = _cuda(z[2], np.int32) if counts else None
        self.rejected = torch.full((1,), z[3], dtype=torch.int64, device="cuda") if rejected else None

    def result(self):
        torch.cuda.synchronize()
        return {"sums": self.sums.cpu().numpy(), "moments": None if self.moments is None else self.moments.cpu().numpy(),
                "counts": None if self.counts is None else self.counts.cpu().numpy(),
                "rejected": None if self.rejected is None else int(self.rejected.item())}


def _deposit(ctx, buf, c, p, max_value=1.0, index=None):
    ctx.deposit(_cuda(c), _cuda(p, np.int32), buf.sums, buf.moments, buf.counts, index, max_value, buf.rejected)


@pytest.fixture(scope="module")
def ctx(tor):
    c = tor.Context(0)
    c.upload(tor.random_scene(0xFACADE).list())
    return c


@pytest.fixture(scope="module")
def cam(tor):
    return tor.camera()


@pytest.fixture(scope="module")
def open_samples(tor, ctx, cam):
    """Samples [3, 8) of every pixel through the open pipeline: (colours (n, 3), pixels (n,) int32), camera order, computed once."""
    rays, rng = ctx.camera_rays(cam, NROWS, NCOLS, first_sample=3, n_samples=5)
    colors = ctx.radiance(rays, rng, DEPTH)[0]
    pixels = torch.arange(NROWS * NCOLS, dtype=torch.int32, device="cuda").repeat_interleave(5)
    torch.cuda.synchronize()
    return colors, pixels


def _progressive(tor, ctx, cam, first, n):
    pg = tor.Progressive(ctx, cam, NROWS, NCOLS, DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE), moments=True)
    pg.samples = first
    pg.add(n)
    torch.cuda.synchronize()
    return pg


def _same_bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.int64), b.reshape(-1).view(torch.int64))


# ---- identity with the closed integrator ---------------------------------------------------------------------------------------

def test_open_pipeline_equals_the_closed_integrator(tor, ctx, cam, open_samples):
    colors, pixels = open_samples
    n = int(colors.shape[0])
    want = _progressive(tor, ctx, cam, 3, 5)
    assert float(want.sums.max()) > 0.0 and float(want.moments.max()) > 0.0

    def check(what, fill):
        sums, moments = torch.zeros_like(want.sums), torch.zeros_like(want.moments)
        rejected = torch.zeros(1, dtype=torch.int64, device="cuda")
        fill(sums, moments, rejected)
        torch.cuda.synchronize()
        assert int(rejected.item()) == 0, what
        assert _same_bits(sums, want.sums), f"{what}: sums differ from tor_render_accumulate_device's"
        assert _same_bits(moments, want.moments), f"{what}: moments differ from tor_render_accumulate_device's"

    check("one call", lambda s, m, r: ctx.deposit(colors, pixels, s, m, rejected=r, max_value=1.0))
    cut = 64 * 7 + 3   # inside a wave and inside a pixel's five samples

    def split(s, m, r):
        ctx.deposit(colors[:cut].contiguous(), pixels[:cut].contiguous(), s, m, rejected=r)
        ctx.deposit(colors[cut:].contiguous(), pixels[cut:].contiguous(), s, m, rejected=r)
    check("two calls", split)
    o = torch.randperm(n, generator=torch.Generator().manual_seed(1)).cuda()
    check("shuffled", lambda s, m, r: ctx.deposit(colors[o].contiguous(), pixels[o].contiguous(), s, m, rejected=r))
    check("shuffled through a list", lambda s, m, r: ctx.deposit(colors, pixels, s, m, index=o.int(), rejected=r))


def test_deposit_on_top_of_the_librarys_own_pass(tor, ctx, cam, open_samples):
    colors, pixels = open_samples
    first = _progressive(tor, ctx, cam, 0, 3)            # Progressive.add(3)
    want = _progressive(tor, ctx, cam, 0, 8)             # Progressive.add(8)
    ctx.deposit(colors, pixels, first.sums, first.moments)
    torch.cuda.synchronize()
    assert _same_bits(first.sums, want.sums) and _same_bits(first.moments, want.moments)


# ---- synthetic entries against the restatement ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plain_ctx(tor):
    return tor.Context(0)    # a deposit reads no scene: none uploaded


@pytest.mark.parametrize("max_value", I.MAX_VALUES)
@pytest.mark.parametrize("name", I.CASES)
def test_synthetic_entries_equal_the_restatement(plain_ctx, name, max_value):
    c, p = I.case(name, max_value)
    want = D.agree(c, p, I.NPIX, max_value)
    buf = Buffers(I.NPIX)
    _deposit(plain_ctx, buf, c, p, max_value)
    got = buf.result()
    print(name, max_value, "rejected", got["rejected"], "deposited", int(got["counts"].sum()))
    assert not D.mismatches(got, want), f"{name}, max_value {max_value}: {D.mismatches(got, want)}"
    if max_value < 128.0:   # ... and on top of what an earlier deposit left, in another order (at 128 a second one leaves the bound)
        o = np.random.default_rng(2).permutation(I.N)
        buf2 = Buffers(I.NPIX, into=want)
        _deposit(plain_ctx, buf2, c[o], p[o], max_value)
        want2 = D.agree(c, p, I.NPIX, max_value, into=want)
        assert not D.mismatches(buf2.result(), want2), f"{name}, max_value {max_value}, second deposit"


def test_lists(plain_ctx):
    for name, idx in I.list_cases().items():
        for case in ("runs", "rejects", "edges"):
            c, p = I.case(case, 1.0)
            want = D.agree(c, p, I.NPIX, 1.0, index=idx)
            buf = Buffers(I.NPIX)
            _deposit(plain_ctx, buf, c, p, 1.0, index=_cuda(idx, np.int32))
            got = buf.result()
            assert not D.mismatches(got, want), f"list '{name}' over '{case}': {D.mismatches(got, want)}"
            if name == "empty":
                assert not got["sums"].any() and not got["counts"].any() and got["rejected"] == 0


def test_optional_buffers(plain_ctx):
    c, p = I.case("rejects", 1.0)
    want = D.agree(c, p, I.NPIX, 1.0)
    assert want["rejected"] > 0
    for off in ("moments", "counts", "rejected"):
        kw = {off: False}
        buf = Buffers(I.NPIX, **kw)
        _deposit(plain_ctx, buf, c, p)
        got = buf.result()
        fields = [f for f in ("sums", "moments", "counts", "rejected") if f != off]
        assert not D.mismatches(got, want, fields), (off, D.mismatches(got, want, fields))
    # buffers that are not named are not touched; a counter holding 7 ends at 7 plus the rejections
    buf = Buffers(I.NPIX)
    buf.rejected.fill_(7)
    plain_ctx.deposit(_cuda(c), _cuda(p, np.int32), buf.sums, None, None, None, 1.0, buf.rejected)
    torch.cuda.synchronize()
    assert int(buf.rejected.item()) == 7 + want["rejected"]
    assert not D.mismatches({"sums": buf.sums.cpu().numpy()}, want, ["sums"])
    assert not buf.moments.any() and not buf.counts.any()


def test_scale_camera_order_equals_random_order_and_the_integer_statement(plain_ctx):
    """On the device only: 2^20 samples, 4096 pixels, 256 per pixel (within the bound at max_value = 1)."""
    n, npix, k = 1 << 20, 4096, 256
    g = torch.Generator(device="cuda").manual_seed(7)
    colors = torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=g) * 1.25
    pixels = torch.arange(npix, dtype=torch.int32, device="cuda").repeat_interleave(k)
    o = torch.randperm(n, device="cuda", generator=g)

    def run(c, p):
        s, m = torch.zeros((npix, 3), dtype=torch.float64, device="cuda"), torch.zeros((npix, 3), dtype=torch.float64, device="cuda")
        cnt, rej = torch.zeros(npix, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        plain_ctx.deposit(c, p, s, m, cnt, None, 1.0, rej)
        return s, m, cnt, rej
    a = run(colors, pixels)
    b = run(colors[o].contiguous(), pixels[o].contiguous())
    torch.cuda.synchronize()
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and torch.equal(a[2], b[2])
    assert int(a[3].item()) == 0 and int(b[3].item()) == 0 and bool((a[2] == k).all())
    # the integer statement in torch: round half to even, int64 sums, scaled back
    qi = torch.round(torch.clamp(colors, max=1.0) * 2.0 ** 36).to(torch.int64)
    q = qi.to(torch.float64) * 2.0 ** -36
    mi = torch.round((q * q) * 2.0 ** 36).to(torch.int64)
    si = torch.zeros((npix, 3), dtype=torch.int64, device="cuda").index_add_(0, pixels.long(), qi)
    mo = torch.zeros((npix, 3), dtype=torch.int64, device="cuda").index_add_(0, pixels.long(), mi)
    assert int(si.max()) < 2 ** 53 and int(mo.max()) < 2 ** 53
    assert _same_bits(a[0], si.to(torch.float64) * 2.0 ** -36) and _same_bits(a[1], mo.to(torch.float64) * 2.0 ** -36)


# ---- Film ----------------------------------------------------------------------------------------------------------------------

def test_film_passes_equal_progressive(tor, ctx, cam):
    pg = tor.Progressive(ctx, cam, NROWS, NCOLS, DEPTH, tor.make_options(seeding=tor.SEED_SAMPLE), moments=True)
    pg.add(3).add(5)
    film = tor.Film(ctx, NROWS, NCOLS, moments=True, max_depth=DEPTH)
    film.add_pass(cam, 3).add_pass(cam, 5, chunk_pixels=37)     # 37 does not divide the 384 pixels
    torch.cuda.synchronize()
    assert film.samples == pg.samples == 8 and film.rejected() == 0 and film.check_budget() == 8
    assert _same_bits(film.sums, pg.sums) and _same_bits(film.moments, pg.moments)
    assert film.noise() == pg.noise()
    assert _same_bits(film.image(2.2), pg.image(2.2))
    # a checkpoint resumes to the same film
    back = tor.Film.from_state(ctx, film.state())
    assert back.samples == 8 and back.uniform and back.max_depth == DEPTH and back.moments is not None and back.counts is None
    assert _same_bits(back.sums, film.sums) and _same_bits(back.moments, film.moments)
    back.add_pass(cam, 2)
    pg.add(2)
    torch.cuda.synchronize()
    assert _same_bits(back.sums, pg.sums) and _same_bits(back.image(), pg.image())


def test_film_lit_pass_equals_the_restatement(tor, ctx, cam):
    n_obj = len(tor.random_scene(0xFACADE))
    emission = np.zeros((n_obj, 3))
    emission[::7] = [6.0, 2.5, 0.75]       # above 1, and above max_value = 4 in one channel
    emission[3::11] = [0.0, 1.5, 3.0]
    seen = []

    def tracer(rays, rng):
        colors = ctx.trace(rays, rng, max_depth=DEPTH, emission=emission)[0]
        seen.append(colors.clone())
        return colors
    k = 2
    film = tor.Film(ctx, NROWS, NCOLS, moments=True, counts=True, max_value=4.0, max_depth=DEPTH)
    film.add_pass(cam, k, tracer=tracer, chunk_pixels=200)
    torch.cuda.synchronize()
    colors = torch.cat(seen).cpu().numpy()
    assert colors.shape == (NROWS * NCOLS * k, 3) and colors.max() > 4.0 and colors.min() >= 0.0
    pixels = np.repeat(np.arange(NROWS * NCOLS), k)
    want = D.agree(colors, pixels, NROWS * NCOLS, 4.0)
    got = {"sums": film.sums.cpu().numpy(), "moments": film.moments.cpu().numpy(), "counts": film.counts.cpu().numpy(),
           "rejected": film.rejected()}
    assert film.rejected() == 0 and not D.mismatches(got, want), D.mismatches(got, want)
    assert want["sums"].max() > 1.0 * k      # the lamps are in the picture
    sums = _cuda(want["sums"])                # image(): tor_resolve_device on the restated sums at k samples
    ref = torch.empty_like(sums)
    ctx.resolve_device(sums.data_ptr(), sums.numel(), k, 2.2, ref.data_ptr(), torch.cuda.current_stream().cuda_stream)
    img = film.image(2.2)
    torch.cuda.synchronize()
    assert _same_bits(img, ref) and float(img.max()) > 1.0


def test_film_splat_with_counts(tor, plain_ctx):
    rng = np.random.default_rng(4)
    nrows, ncols = 6, 9
    npix = nrows * ncols
    n = 700
    p = rng.integers(0, npix - 10, size=n).astype(np.int32)      # the last ten pixels stay empty
    c = rng.uniform(0.0, 1.2, size=(n, 3))
    c[5] = [np.nan, 0.1, 0.1]
    film = tor.Film(plain_ctx, nrows, ncols, moments=True, counts=True)
    film.deposit(p[:300], _cuda(c[:300])).deposit(_cuda(p[300:], np.int32), _cuda(c[300:]))
    want = D.agree(c, p, npix, 1.0)
    got = {"sums": film.sums.cpu().numpy(), "moments": film.moments.cpu().numpy(), "counts": film.counts.cpu().numpy(),
           "rejected": film.rejected()}
    assert not D.mismatches(got, want) and film.rejected() == 1 and not film.uniform
    assert len(set(want["counts"].tolist())) > 3 and (want["counts"][-10:] == 0).all()
    # image(): tor_resolve_counts_device on the restated sums, a pixel without samples at count 1 -- black
    sums, counts = _cuda(want["sums"]), _cuda(np.maximum(want["counts"], 1), np.int32)
    ref = torch.empty_like(sums)
    plain_ctx.resolve_counts_device(sums.data_ptr(), counts.data_ptr(), npix, 2.2, ref.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    img = film.image(2.2)
    torch.cuda.synchronize()
    assert _same_bits(img, ref) and not img.reshape(-1, 3)[-10:].any() and float(img.max()) > 0.0
    assert (film.counts.cpu().numpy().reshape(-1)[-10:] == 0).all()        # the film's own counts keep their zeros
    with pytest.raises(tor.TorError, match="unequal"):
        film.noise()
    back = tor.Film.from_state(plain_ctx, film.state())
    assert not back.uniform and back.rejected() == 1 and torch.equal(back.counts, film.counts) and _same_bits(back.image(), img)


def test_film_check_budget_raises_past_the_bound(tor, plain_ctx):
    film = tor.Film(plain_ctx, 2, 2, counts=True, max_value=128.0)
    assert film.budget() == 8                                   # 2^17 / 128^2
    film.deposit(np.zeros(8, dtype=np.int32), _cuda(np.full((8, 3), 0.5)))
    assert film.check_budget() == 8
    film.deposit(np.zeros(1, dtype=np.int32), _cuda(np.full((1, 3), 0.5)))
    with pytest.raises(tor.TorError, match="exactness bound"):
        film.check_budget()
    uni = tor.Film(plain_ctx, 2, 2, max_value=1.0)
    assert uni.budget() == 1 << 17
    uni.samples = (1 << 17) + 1                                 # uniform passes: the sample count is what is checked
    with pytest.raises(tor.TorError, match="exactness bound"):
        uni.check_budget()
    assert tor.Film(plain_ctx, 2, 2, max_value=0.25).budget() == 1 << 19
