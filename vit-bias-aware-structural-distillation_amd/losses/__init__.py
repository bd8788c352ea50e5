from .combined import BASDLoss, _align_token_count  # noqa: F401
from .layer_selector import (GrassmannianLayerSelector, marchenko_pastur_rank, marchenko_pastur_rank_wide,  # noqa: F401
                             mp_rank_route)
from .relational import geometric_relational_loss  # noqa: F401
