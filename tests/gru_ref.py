"""fp64 statements, in torch on the CPU, of what the GRU / RNN kernels compute: both cells (nn.GRUCell / nn.RNNCell layout: weights
[3H][H] / [H][H], gate order r, z, n), the step of the reference's `gru` / `rnn` modules (lstm.py:75-136), the teacher-forced
sequence, and the hand-written backward of the GRU cell (dvg_gru_gates_bwd's formulas + the GEMMs around it).

Planted defects (`defect=`) - each is a plausible slip, and tests/test_gru_host.py shows that the bars of the GPU tests catch it:
  forward   "bhn_outside"   b_hn added outside the r * product (as if it could be folded into the input half like the LSTM's b_hh)
            "order_rnz"     the weight slices read in the order r, n, z
            "z_swapped"     z and 1 - z exchanged in the state update
  backward  "dgh_no_r"      the hidden side's n slice without its factor r
            "dhprev_no_dz"  dh_prev without the direct term d * z
"""
import torch

FORWARD_DEFECTS = ("bhn_outside", "order_rnz", "z_swapped")
BACKWARD_DEFECTS = ("dgh_no_r", "dhprev_no_dz")


def _f64(*ts):
    return tuple(None if t is None else t.detach().double().cpu() for t in ts)


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, defect=None):
    """(h', acts) with acts = cat(r, z, n, hn) (B, 4H); dtype follows the inputs (fp64 in the tests, any dtype under autograd)."""
    H = h.shape[1]
    gi = x @ w_ih.t() + b_ih
    gh = h @ w_hh.t()
    order = (0, 2, 1) if defect == "order_rnz" else (0, 1, 2)
    sl = [slice(k * H, (k + 1) * H) for k in order]
    r = torch.sigmoid(gi[:, sl[0]] + gh[:, sl[0]] + b_hh[sl[0]])
    z = torch.sigmoid(gi[:, sl[1]] + gh[:, sl[1]] + b_hh[sl[1]])
    if defect == "bhn_outside":
        hn = gh[:, sl[2]]
        n = torch.tanh(gi[:, sl[2]] + b_hh[sl[2]] + r * hn)
    else:
        hn = gh[:, sl[2]] + b_hh[sl[2]]
        n = torch.tanh(gi[:, sl[2]] + r * hn)
    h2 = z * n + (1 - z) * h if defect == "z_swapped" else (1 - z) * n + z * h
    return h2, torch.cat([r, z, n, hn], 1)


def rnn_cell(x, h, w_ih, w_hh, b_ih, b_hh):
    return torch.tanh(x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh)


def gates_bwd(d, acts, h_prev, defect=None):
    """dvg_gru_gates_bwd: (dGi, dGh, dh_prev = d z) from d = dh_a + dh_b, acts (B, 4H) and h_prev (None: zeros)."""
    H = acts.shape[1] // 4
    r, z, n, hn = (acts[:, k * H:(k + 1) * H] for k in range(4))
    h = torch.zeros_like(d) if h_prev is None else h_prev
    da_n = d * (1 - z) * (1 - n * n)
    da_r = da_n * hn * r * (1 - r)
    da_z = d * (h - n) * z * (1 - z)
    dGi = torch.cat([da_r, da_z, da_n], 1)
    dGh = torch.cat([da_r, da_z, da_n if defect == "dgh_no_r" else da_n * r], 1)
    dh_prev = torch.zeros_like(d) if defect == "dhprev_no_dz" else d * z
    return dGi, dGh, dh_prev


def gru_cell_backward(d, x, h, w_ih, w_hh, acts, defect=None):
    """The whole hand-written backward of one cell: dx, dh, dW_ih, dW_hh, db_ih, db_hh."""
    dGi, dGh, dh = gates_bwd(d, acts, h, defect)
    return {"x": dGi @ w_ih, "h": dh + dGh @ w_hh, "w_ih": dGi.t() @ x, "w_hh": dGh.t() @ h, "b_ih": dGi.sum(0),
            "b_hh": dGh.sum(0)}


def rnn_cell_backward(d, x, h, w_ih, w_hh, h2):
    """tanh' then the GEMMs (what _RNNCell composes from act_bwd, gemm_nt and gemm_tn)."""
    dpre = d * (1 - h2 * h2)
    return {"x": dpre @ w_ih, "h": dpre @ w_hh, "w_ih": dpre.t() @ x, "w_hh": dpre.t() @ h, "b_ih": dpre.sum(0),
            "b_hh": dpre.sum(0)}


def init_hidden(B, H, n_layers, dtype=torch.float64):
    return [torch.zeros(B, H, dtype=dtype) for _ in range(n_layers)]


def module_step(x, sd, hidden, kind):
    """One call of lstm.gru / lstm.rnn (lstm.py:97-104,129-136) on a state_dict `sd`; `hidden` (a list of tensors) is updated in
    place, as the module's attribute is."""
    h_in = x.reshape(-1, sd["embed.weight"].shape[1]) @ sd["embed.weight"].t() + sd["embed.bias"]
    for i in range(len(hidden)):
        p = [sd[f"{kind}.{i}.{k}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        hidden[i] = gru_cell(h_in, hidden[i], *p)[0] if kind == "gru" else rnn_cell(h_in, hidden[i], *p)
        h_in = hidden[i]
    return torch.tanh(h_in @ sd["output.0.weight"].t() + sd["output.0.bias"])


def sequence(xs, sd, kind, n_layers):
    """[module(x) for x in xs] from the zero state: (S, B, out)."""
    hidden = init_hidden(xs.shape[1], sd["embed.weight"].shape[0], n_layers, xs.dtype)
    return torch.stack([module_step(xs[t], sd, hidden, kind) for t in range(xs.shape[0])])


def bptt(sd, xs, ws, kind, n_layers, dtype=torch.float64):
    """Autograd of sum(sequence(xs) * ws) in `dtype`: (y, {parameter name: gradient, "x": input gradient})."""
    leaf = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = xs.detach().to(dtype).clone().requires_grad_(True)
    y = sequence(x, leaf, kind, n_layers)
    (y * ws.detach().to(dtype)).sum().backward()
    g = {k: v.grad for k, v in leaf.items()}
    g["x"] = x.grad
    return y.detach(), g
