"""TEST-ONLY float64 reference of the pairwise sigmoid loss: torch autograd over exp(theta) * I_hat T_hat^T + b with
F.logsigmoid, plain and keyed -- nothing of the package is imported.  Every call asserts the closed forms of the gradients and the
identity with F.binary_cross_entropy_with_logits(reduction="sum") / Bg.  Also the float64 restatement of what the fused kernel
writes for one block.  theta and b are taken as the fp32 values the device holds (pass `float(torch.tensor(v, dtype=float32))`)."""
import torch
import torch.nn.functional as F


def positives(rows, cols, off=0, keys_row=None, keys_col=None):
    """bool [rows, cols]: column off + i of row i, or, with keys, the columns whose key equals the row's"""
    if keys_row is None:
        return torch.arange(cols)[None, :] == (torch.arange(rows) + off)[:, None]
    return keys_row[:, None] == keys_col[None, :]


def closed_form(x, pos):
    """float64 (l, g) per element: l = softplus(-x) | softplus(x), g = -sigmoid(-x) | sigmoid(x) (never sigmoid(x) - 1)"""
    l = torch.where(pos, F.softplus(-x), F.softplus(x))
    g = torch.where(pos, -torch.sigmoid(-x), torch.sigmoid(x))
    return l, g


def sigmoid_grads(img, txt, theta, bias, keys=None):
    """{"loss", "dtheta", "db" (floats), "dimg", "dtxt" (float64), "mag_theta" = sum |g (x - b)| / Bg, "mag_b" = sum |g| / Bg (the
    scales of the summands of d theta and d b), "x", "g"} over the whole batch"""
    Bg = img.shape[0]
    i64 = img.detach().double().requires_grad_(True)
    t64 = txt.detach().double().requires_grad_(True)
    th = torch.tensor(float(theta), dtype=torch.float64, requires_grad=True)
    b = torch.tensor(float(bias), dtype=torch.float64, requires_grad=True)
    C = F.normalize(i64, dim=1) @ F.normalize(t64, dim=1).T
    C.retain_grad()
    x = torch.exp(th) * C + b
    pos = positives(Bg, Bg) if keys is None else positives(Bg, Bg, 0, keys, keys)
    z = torch.where(pos, x, -x)
    loss = -F.logsigmoid(z).sum() / Bg
    loss.backward()
    xd, t, loss = x.detach(), float(torch.exp(th.detach())), loss.detach()
    l, g = closed_form(xd, pos)
    tol = 1e-12
    bce = F.binary_cross_entropy_with_logits(xd, pos.double(), reduction="sum") / Bg
    assert abs(float(loss) - float(bce)) <= tol * max(1.0, abs(float(bce))), (float(loss), float(bce))        # the issue's identity
    assert abs(float(loss) - float(l.sum() / Bg)) <= tol * max(1.0, float(l.sum() / Bg))
    mag_theta, mag_b = float((g * (xd - b.detach())).abs().sum() / Bg), float(g.abs().sum() / Bg)
    torch.testing.assert_close(C.grad, t * g / Bg, rtol=1e-12, atol=1e-15)                                    # dL/dC = t g / Bg
    assert abs(float(th.grad) - float((g * (xd - b.detach())).sum() / Bg)) <= tol * max(1.0, mag_theta)       # dL/dtheta
    assert abs(float(b.grad) - float(g.sum() / Bg)) <= tol * max(1.0, mag_b)                                  # dL/db
    return {"loss": float(loss), "dimg": i64.grad, "dtxt": t64.grad, "dtheta": float(th.grad), "db": float(b.grad),
            "mag_theta": mag_theta, "mag_b": mag_b, "x": xd, "g": g, "pos": pos}


def block(C, theta, bias, off=0, keys_row=None, keys_col=None):
    """float64 of one block: (t * g, l, g * (t c), g), each [rows, cols]: what the fused kernel leaves in C and the summands of
    its three planes of partial sums"""
    t = torch.exp(torch.tensor(float(theta), dtype=torch.float64))
    c = C.double()
    x = t * c + float(bias)
    pos = positives(C.shape[0], C.shape[1], off, keys_row, keys_col)
    l, g = closed_form(x, pos)
    return t * g, l, g * (t * c), g


def block_fp32(C, theta, bias, off=0, keys_row=None, keys_col=None):
    """the same four quantities by the kernel's formulas in fp32 on the CPU: e = exp(-|x|), r = 1 / (1 + e), x = fma(t, c, b)"""
    t = torch.exp(torch.tensor(float(theta), dtype=torch.float32))
    b = torch.tensor(float(bias), dtype=torch.float32)
    c = C.float()
    x = (t.double() * c.double() + b.double()).float()     # fma: the product is exact in float64, one rounding to fp32 follows the sum
    pos = positives(C.shape[0], C.shape[1], off, keys_row, keys_col)
    e = torch.exp(-x.abs())
    r = 1.0 / (1.0 + e)
    er = e * r
    ge = x >= 0
    g = torch.where(pos, -torch.where(ge, er, r), torch.where(ge, r, er))
    y = torch.where(pos, -x, x)
    l = torch.where(y > 0, y, torch.zeros_like(y)) + torch.log1p(e)
    return t * g, l, g * (t * c), g
