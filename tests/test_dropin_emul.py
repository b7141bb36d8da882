import pytest

import dropin_cases as dc


@pytest.mark.parametrize("R", [8, 14])
def test_reference_style_usage(R):
    assert dc.case_reference_style_usage("emul", R)


def test_training_loop():
    assert dc.case_training_loop("emul") >= 1


def test_add_dirichlet_noise_mirror():
    """MCTS.add_dirichlet_noise (reference mcts.py:45-56, defined but unused there too): a convex blend
    of each policy row with a Dirichlet sample over the whole action space."""
    import numpy as np
    import torch
    dc.setup("emul", 8)
    from four_player_chess_board import FourPlayerChess
    from mcts import MCTS
    A = FourPlayerChess.action_space_size
    pol = torch.softmax(torch.arange(3 * A, dtype=torch.float32).reshape(3, A) % 13, dim=1)
    m = MCTS(FourPlayerChess, lambda x: None, {"C": 3, "num_searches": 1, "dirichlet_alpha": 0.3, "dirichlet_epsilon": 0.25})
    np.random.seed(0)
    out = m.add_dirichlet_noise(pol, "cpu")
    assert out.shape == pol.shape and out.dtype == torch.float32
    assert torch.allclose(out.sum(1), torch.ones(3), atol=1e-5) and (out >= 0).all()
    assert ((out - 0.75 * pol) >= -1e-7).all() and not torch.equal(out, pol)
    m.args["dirichlet_epsilon"] = 0.0
    assert torch.equal(m.add_dirichlet_noise(pol, "cpu"), pol)


def test_host_node_forms_reproduce_reference_searches():
    """Node.ChooseLeaf / SelectChild / Backpropagate(Nodes) / ExpandNodes as host methods (wrapper.cpp:233-253):
    a per-simulation search driven through them reproduces the reference's golden visit counts."""
    assert dc.case_host_tree("emul", 8, max_cases=2, max_sims=100) >= 1


@pytest.mark.parametrize("R", [8, 14])
def test_play_loop_takes_successors_from_one_batched_prefetch(R):
    assert dc.case_play_loop_prefetch("emul", R) >= 6


@pytest.mark.parametrize("R", [8, 14])
def test_attacked_square_methods_of_the_binding_surface(R):
    assert dc.case_attacked_square_methods("emul", R, max_cases=10) >= 10
