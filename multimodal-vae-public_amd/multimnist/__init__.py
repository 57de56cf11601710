from . import model  # noqa: F401
from . import utils  # noqa: F401
from . import datasets  # noqa: F401
