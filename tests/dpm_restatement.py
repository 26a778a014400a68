"""Test-local restatement of DPM-Solver++ multistep (Lu et al. 2022, arXiv 2211.01095, Alg. 2) in the tensor form of diffusers
>=0.15's DPMSolverMultistepScheduler: fp32 torch on the CPU, 0-d tensors for the scalars, the expressions written out literally
(not through the product's coefficient plan), so the product's kernel is checked against the published update in its op order."""
import torch


def tables(ac):
    """alpha_t, sigma_t, lambda_t from alphas_cumprod."""
    alpha_t = torch.sqrt(ac)
    sigma_t = torch.sqrt(1 - ac)
    return alpha_t, sigma_t, torch.log(alpha_t) - torch.log(sigma_t)


def orders(n, solver_order, lower_order_final=True):
    out = []
    for i in range(n):
        low = lower_order_final and n < 15
        if solver_order == 1 or i == 0 or (low and i == n - 1):
            out.append(1)
        elif solver_order == 2 or i == 1 or (low and i == n - 2):
            out.append(2)
        else:
            out.append(3)
    return out


def data_prediction(tab, s0, x, out, vpred):
    al, sg, _ = tab
    alpha_s0, sigma_s0 = al[s0], sg[s0]
    return alpha_s0 * x - sigma_s0 * out if vpred else (x - sigma_s0 * out) / alpha_s0


def step(tab, ts, i, x, out, hist, order, solver_type="midpoint", vpred=False):
    """Step i of the grid `ts` (int list): returns (x_t, m0); hist = the m0 of the earlier steps (last = previous step)."""
    al, sg, lam = tab
    s0 = int(ts[i]); t = int(ts[i + 1]) if i + 1 < len(ts) else 0
    alpha_t, sigma_t, lambda_t = al[t], sg[t], lam[t]
    alpha_s0, sigma_s0, lambda_s0 = al[s0], sg[s0], lam[s0]
    m0 = data_prediction(tab, s0, x, out, vpred)
    h = lambda_t - lambda_s0
    if order == 1:
        x_t = (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * m0
    elif order == 2:
        m1 = hist[-1]
        lambda_s1 = lam[int(ts[i - 1])]
        h_0 = lambda_s0 - lambda_s1
        r0 = h_0 / h
        D0, D1 = m0, (1.0 / r0) * (m0 - m1)
        if solver_type == "midpoint":
            x_t = (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * D0 - 0.5 * (alpha_t * (torch.exp(-h) - 1.0)) * D1
        else:
            x_t = (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * D0 + (alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) * D1
    else:
        m1, m2 = hist[-1], hist[-2]
        lambda_s1, lambda_s2 = lam[int(ts[i - 1])], lam[int(ts[i - 2])]
        h_0, h_1 = lambda_s0 - lambda_s1, lambda_s1 - lambda_s2
        r0, r1 = h_0 / h, h_1 / h
        D0 = m0
        D1_0, D1_1 = (1.0 / r0) * (m0 - m1), (1.0 / r1) * (m1 - m2)
        D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
        D2 = (1.0 / (r0 + r1)) * (D1_0 - D1_1)
        x_t = ((sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * D0 + (alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) * D1
               - (alpha_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5)) * D2)
    return x_t, m0


class Gaussian:
    """Data x0 ~ N(mu, I): the exact eps-predictor is sigma_t (x - alpha_t mu) / (alpha_t^2 + sigma_t^2), and
    (x - alpha_t mu) / sqrt(alpha_t^2 + sigma_t^2) is invariant along the probability-flow ODE, so the exact solution at t = 0
    is known in closed form."""

    def __init__(self, tab, T, numel=4096, seed=0):
        g = torch.Generator().manual_seed(seed)
        al, sg, _ = tab
        self.tab = tab
        self.mu = torch.randn(numel, generator=g) * 0.5 + 1.0
        aT, sT = al[T], sg[T]
        self.xT = aT * self.mu + torch.sqrt(aT ** 2 + sT ** 2) * torch.randn(numel, generator=g)
        a0, s0 = al[0], sg[0]
        self.exact = a0 * self.mu + (self.xT - aT * self.mu) * torch.sqrt(a0 ** 2 + s0 ** 2) / torch.sqrt(aT ** 2 + sT ** 2)

    def eps(self, x, t, mu=None):
        al, sg, _ = self.tab
        a, s = al[t], sg[t]
        mu = self.mu if mu is None else mu
        return s * (x - a * mu) / (a * a + s * s)

    def rel_err(self, x):
        x = x.detach().float().cpu().reshape(-1)
        return float((x - self.exact).norm() / self.exact.norm())
