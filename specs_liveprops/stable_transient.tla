------------------------------ MODULE stable_transient ------------------------------
(* The twin of stable whose ~P state is transient: b = 0 is left by the one step of a fair process (its one-state component is unfair: the process is enabled there), and the behaviour ends in b = 1, so  <>[](b = 1)  HOLDS. *)
EXTENDS Naturals

(* --algorithm stable_transient
variables b = 0;

fair process Up = 0
begin
  U: b := 1;
end process

end algorithm *)

Settles == <>[](b = 1)
=============================================================================
