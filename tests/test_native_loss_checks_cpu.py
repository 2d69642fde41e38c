"""CPU: the host checks of the fused objectives' wrappers in ctdd.native (ctelbo_loss*, crm_loss*, score_elbo_loss*, masked or not).
One operand at a time is mis-shaped -- a state (B, D + 1), a table (B, S, S + 1), 2-D logits, a wrong grad_out -- and the call must
raise a CtddError that names that operand; these are CPU tensors, so the error comes before anything could reach a device.
Correctly shaped CPU tensors still get the "must live on a GPU" refusal."""
import re

import pytest
import torch

B, D, S = 2, 3, 4
K = 2                   # the window wrapper reads rows [K, K + D) of (B, K + D, S) logits


def _operands():
    st = lambda: torch.zeros(B, D, dtype=torch.int32)
    tab = lambda: torch.zeros(B, S, S)
    return dict(logits=torch.zeros(B, D, S), x0=st(), xt=st(), x_tilde=st(), reg_x=st(), qt0=tab(), qt0T=tab(), rate=tab(),
                free=torch.ones(B, D, dtype=torch.bool), grad_out=None)


# name -> (call(native, operands), name of the (B, D, S) operand, states, tables, takes grad_out)
WRAPPERS = {
    "ctelbo_loss": (lambda n, o: n.ctelbo_loss(o["logits"], o["x0"], o["x_tilde"], o["qt0"], o["qt0T"], o["rate"], 1e-9, 1.0, 0.1),
                    "logits", ("x0", "x_tilde"), ("qt0", "qt0T", "rate"), False),
    "ctelbo_loss[terms]": (lambda n, o: n.ctelbo_loss(o["logits"], o["x0"], o["x_tilde"], o["qt0"], o["qt0T"], o["rate"], 1e-9, 1.0, 0.1,
                                                      reg_scale=0.5),
                           "logits", ("x0", "x_tilde"), ("qt0", "qt0T", "rate"), False),
    "ctelbo_loss_window": (lambda n, o: n.ctelbo_loss_window(o["logits"], o["x0"], o["x_tilde"], o["qt0"], o["qt0T"], o["rate"], 1e-9, 1.0,
                                                             1.0, 0.1, K, grad_out=o["grad_out"]),
                           "logits", ("x0", "x_tilde"), ("qt0", "qt0T", "rate"), True),
    "ctelbo_loss_masked": (lambda n, o: n.ctelbo_loss_masked(o["logits"], o["x0"], o["x_tilde"], o["free"], o["qt0"], o["qt0T"], o["rate"],
                                                             1e-9, 1.0, 1.0, 0.1, grad_out=o["grad_out"]),
                           "logits", ("x0", "x_tilde"), ("qt0", "qt0T", "rate"), True),
    "crm_loss": (lambda n, o: n.crm_loss(o["logits"], o["xt"], o["x0"], o["qt0"], "elbo", 0.5, 0.1), "logits", ("xt", "x0"), ("qt0",), False),
    "crm_loss_ll": (lambda n, o: n.crm_loss_ll(o["logits"], o["xt"], o["qt0"], "elbo", 0.5), "ll_all", ("xt",), ("qt0",), False),
    "crm_loss_masked": (lambda n, o: n.crm_loss_masked(o["logits"], o["xt"], o["x0"], o["free"], o["qt0"], "elbo", 0.5, 0.1,
                                                       grad_out=o["grad_out"]), "logits", ("xt", "x0"), ("qt0",), True),
    "crm_loss_ll_masked": (lambda n, o: n.crm_loss_ll_masked(o["logits"], o["xt"], o["free"], o["qt0"], "elbo", 0.5, grad_out=o["grad_out"]),
                           "ll_all", ("xt",), ("qt0",), True),
    "score_elbo_loss": (lambda n, o: n.score_elbo_loss(o["logits"], o["x0"], o["x_tilde"], o["reg_x"], o["qt0"], o["rate"], 1e-9, 0.1),
                        "logits", ("x0", "x_tilde", "reg_x"), ("qt0", "rate"), False),
    "score_elbo_loss_ll": (lambda n, o: n.score_elbo_loss_ll(o["logits"], o["x0"], o["x_tilde"], o["reg_x"], o["qt0"], o["rate"], 1e-9, 0.1),
                           "ll_all", ("x0", "x_tilde", "reg_x"), ("qt0", "rate"), False),
    "score_elbo_loss_masked": (lambda n, o: n.score_elbo_loss_masked(o["logits"], o["x0"], o["x_tilde"], o["reg_x"], o["free"], o["qt0"],
                                                                     o["rate"], 1e-9, 0.1, grad_out=o["grad_out"]),
                               "logits", ("x0", "x_tilde", "reg_x"), ("qt0", "rate"), True),
    "score_elbo_loss_ll_masked": (lambda n, o: n.score_elbo_loss_ll_masked(o["logits"], o["x0"], o["x_tilde"], o["reg_x"], o["free"],
                                                                           o["qt0"], o["rate"], 1e-9, 0.1, grad_out=o["grad_out"]),
                                  "ll_all", ("x0", "x_tilde", "reg_x"), ("qt0", "rate"), True),
}


def _cases():
    for w, (_, first, states, tables, takes_grad) in WRAPPERS.items():
        for bad in ("logits",) + states + tables + (("grad_out",) if takes_grad else ()):
            yield w, bad


def _prepared(wrapper):
    o = _operands()
    if wrapper == "ctelbo_loss_window":
        o["logits"] = torch.zeros(B, K + D, S)
    return o


@pytest.mark.parametrize("wrapper,bad", list(_cases()))
def test_a_mis_shaped_operand_is_named(wrapper, bad):
    from ctdd import native
    call, first, states, tables, _ = WRAPPERS[wrapper]
    o = _prepared(wrapper)
    if bad == "logits":
        o["logits"], named = torch.zeros(B, S), first
    elif bad in states:
        o[bad], named = torch.zeros(B, D + 1, dtype=torch.int32), bad
    elif bad in tables:
        o[bad], named = torch.zeros(B, S, S + 1), bad
    else:
        o["grad_out"], named = torch.zeros(*o["logits"].shape[:2], S + 1), "grad_out"
    with pytest.raises(native.CtddError) as e:
        call(native, o)
    assert re.search(r"\b" + named + r"\b", str(e.value)), str(e.value)
    assert "must live on a GPU" not in str(e.value)


@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_well_shaped_cpu_tensors_are_refused_as_cpu_tensors(wrapper):
    from ctdd import native
    o = _prepared(wrapper)
    with pytest.raises(native.CtddError, match="must live on a GPU"):
        WRAPPERS[wrapper][0](native, o)
    if WRAPPERS[wrapper][4]:
        o["grad_out"] = torch.zeros_like(o["logits"])
        with pytest.raises(native.CtddError, match="must live on a GPU"):
            WRAPPERS[wrapper][0](native, o)
