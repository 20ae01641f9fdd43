from .retrieval_evaluator import RankingEvaluator  # noqa: F401
from .dev_pool import DevPool  # noqa: F401
from .reranking_evaluator import RerankingEvaluator  # noqa: F401
