"""Float64 reference of the spectral loss term (the c_fft term of L1_freq, Fusion10_freq and L1_ssim_freq) and inputs on which a
float32 transform can be compared with it.  Plain CPU code: torch.fft in float64, autograd for the gradient.

    loss_b = mean over (c, y, x, re / im) of |FFT2(pred) - FFT2(target)|            (hnerv_utils.py:376-385 of the reference)

The gradient of that term carries sign() of every real and imaginary component of the spectrum.  A component that lies within rounding
of zero may take the other sign in float32, and ONE flipped sign moves every pixel of its plane by up to 4 * gscale -- more than the
gradient tolerance on a small frame, for no fault of the kernel under test.  make_inputs therefore pushes every such component of the
difference image away from zero before the inputs are rounded, and reports how many are still close: a condition that the tests assert
to be 0 before they call the library, not a measurement."""
import torch


def spectral_loss_f64(pred, tgt):
    """Per-sample value [B] of the spectral term, float64."""
    pred, tgt = pred.double(), tgt.double()
    return torch.view_as_real(torch.fft.fft2(pred) - torch.fft.fft2(tgt)).abs().flatten(1).mean(1)


def spectral_grad_f64(pred, tgt):
    """d (batch mean of spectral_loss_f64) / d pred, by float64 autograd over the same expression."""
    p = pred.detach().double().requires_grad_(True)
    g, = torch.autograd.grad(spectral_loss_f64(p, tgt).mean(), [p])
    return g


def structural_zeros(H, W):
    """[H, W, 2] bool: the components of the spectrum of a REAL image that are zero by symmetry -- the imaginary parts of the bins that are
    their own conjugate mirror, (0 or H/2, 0 or W/2)."""
    m = torch.zeros(H, W, 2, dtype=torch.bool)
    ys = [0] + ([H // 2] if H % 2 == 0 else [])
    xs = [0] + ([W // 2] if W % 2 == 0 else [])
    for y in ys:
        for x in xs:
            m[y, x, 1] = True
    return m


def _rms(c, free):
    """Root mean square per plane [B, C, 1, 1, 1] of the components of c [B, C, H, W, 2] that are not structurally zero."""
    n = int(free.sum())
    return ((c * c * free).sum(dim=(-3, -2, -1), keepdim=True) / n).sqrt()


def near_zero_census(pred, tgt, tau=1e-4):
    """How many non-structural components of the float64 spectrum of pred - tgt lie within tau * rms (of their plane) of zero."""
    H, W = pred.shape[-2:]
    free = ~structural_zeros(H, W)
    c = torch.view_as_real(torch.fft.fft2(pred.double()) - torch.fft.fft2(tgt.double()))
    return int(((c.abs() < tau * _rms(c, free)) & free).sum())


def make_inputs(shape, seed, tau=1e-4):
    """(pred, tgt, census): float32 [B, C, H, W] images whose difference has no spectral component near zero.

    tgt = rand, d = 0.1 * randn in float64.  Every non-structural real or imaginary component of fft2(d) with |c| < tau * rms becomes
    copysign(2 * tau * rms, c) -- elementwise on the full spectrum: a bin and its mirror hold (re, im) and (re, -im), so both move alike and
    the spectrum stays Hermitian.  The structurally zero components stay zero.  pred = tgt + ifft2(...), both rounded to float32 and NOT
    clamped (neither the spectral term nor L1 needs [0, 1]).  census: near_zero_census of the rounded inputs."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    tgt = torch.rand(shape, generator=g, dtype=torch.float64)
    d = 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
    free = ~structural_zeros(H, W)
    c = torch.view_as_real(torch.fft.fft2(d)).clone()
    lim = tau * _rms(c, free)
    small = (c.abs() < lim) & free
    c = torch.where(small, torch.copysign(2 * lim.expand_as(c), c), c)
    c = torch.where(free, c, torch.zeros_like(c))
    d2 = torch.fft.ifft2(torch.view_as_complex(c.contiguous())).real
    tgt32 = tgt.float()
    pred32 = (tgt + d2).float()
    return pred32, tgt32, near_zero_census(pred32, tgt32, tau)


# The frames of tests/test_gpu_fft_loss.py (and the census test of tests/test_fft_loss_ref_cpu.py), with what each one reaches.
MAIN_CASES = [                       # bnerv_loss_fwd_bwd: generic radices up to 31
    (1, 3, 77, 91),                  # 7*11 x 7*13: a generic stage with j != 0 on both axes; odd W; B*C*H = 231, a lone last row
    (2, 1, 143, 119),                # 11*13 x 7*17; two samples: per-sample sums
    (1, 3, 221, 187),                # 13*17 x 11*17
    (1, 1, 323, 437),                # 17*19 x 19*23
    (1, 1, 667, 899),                # 23*29 x 29*31
    (1, 3, 49, 217),                 # 7*7, a repeated generic radix, x 7*31
    (1, 1, 308, 180),                # 4*7*11: closed-form stages, then two generic ones
    (1, 2, 116, 124),                # 4*29 x 4*31: the two largest radices as the ONE generic stage of an axis (the class of 176 x 208)
    (1, 2, 10, 2560),                # W at the one-batch boundary of the adjoint rows, above 2048 (the tail loop of the table copy)
    (1, 1, 12, 2574),                # 2*3*3*11*13 > 2560: multi-batch adjoint rows with generic stages
    (1, 1, 6, 3840),                 # 4K-wide rows, closed-form radices only, multi-batch
    (1, 1, 2310, 10),                # 2*3*5*7*11 > 2048 as the column length
    (1, 1, 1, 7), (1, 3, 7, 1), (2, 1, 2, 2), (1, 1, 3, 4),      # a side of 1 or 2: no stage at all, one kept column
]
OPERATOR_CASES = MAIN_CASES[:3]      # L1_freq through the operators
LONG_ROW_CASES = [(1, 2, 10, 2560), (1, 1, 12, 2574), (1, 1, 6, 3840), (1, 1, 4, 8000)]      # L1_freq: the adjoint rows ADD to a gradient, in one batch and in several
SSIM_CASES = [                       # bnerv_loss_ssim_fwd_bwd: generic radices up to 37, sides >= 11
    (1, 3, 77, 259),                 # 7*11 x 7*37
    (2, 1, 148, 111),                # 4*37 x 3*37
    (1, 1, 13, 2590),                # 2*5*7*37 > 2560
    (1, 1, 11, 6400),                # close to that path's 128 KB row limit
]
LIMIT_CASES = [(1, 1, 4, 8000), (1, 1, 4000, 4)]      # row and column lengths near the top of what the LDS takes


def case_seed(shape):
    return 1000 + sum(shape)


def radix_class(shape, maxr=31):
    """'closed-form', 'one generic' or 'two generic': the largest number of generic (prime >= 7) stages on either axis."""
    def generic(n):
        k = 0
        for r in (2, 3, 5):
            while n % r == 0:
                n //= r
        for r in range(7, maxr + 1, 2):
            while n % r == 0:
                n //= r
                k += 1
        assert n == 1
        return k
    k = max(generic(shape[2]), generic(shape[3]))
    return ("closed-form", "one generic", "two generic")[min(k, 2)]
