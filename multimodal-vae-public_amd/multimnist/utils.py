"""Drop-in for the reference's ``multimnist/utils.py``: the character set of the text modality (ten digits, a start
symbol ``SOS`` and a fill symbol ``FILL``; strings of at most ``max_length`` = 4 characters) and the conversions
between digit strings and index tensors, with the reference's names, signatures and results.  The constants are the
ones ``model.py`` defines -- one definition, re-exported here."""
import torch

from .model import FILL, SOS, all_characters, max_length, n_characters  # noqa: F401


def char_tensor(string):
    """'17' -> int64 [max_length] = [1, 7, FILL, FILL] (multimnist/utils.py:22-31)."""
    if len(string) > max_length:
        raise IndexError('%r has more than %d characters' % (string, max_length))
    codes = [all_characters.index(ch) for ch in string]      # ValueError on anything but a digit, like the reference
    return torch.tensor(codes + [FILL] * (max_length - len(codes)), dtype=torch.int64)


def charlist_tensor(charlist):
    """[3, 0, 9] (ints or 0-d tensors) -> char_tensor('309') (multimnist/utils.py:34-37)."""
    return char_tensor(''.join(str(int(i)) for i in charlist))


def index_to_char(top_i):
    """One index as text: a digit, '^' for SOS, nothing for FILL (multimnist/utils.py:49-56)."""
    top_i = int(top_i)
    if top_i == FILL:
        return ''
    return '^' if top_i == SOS else all_characters[top_i]


def tensor_to_string(tensor):
    """int64 [length] -> the string of its characters, FILL dropped (multimnist/utils.py:40-46)."""
    return ''.join(index_to_char(tensor[i]) for i in range(tensor.size(0)))
