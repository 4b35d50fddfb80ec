------------------------------ MODULE stable ------------------------------
(* Written to show: <>[]P LOOKS FOR ONE ~P STATE IN A FAIR COMPONENT.  A fair process flips b for ever: the two states are one fair component that holds a P state (b = 1) and a ~P state (b = 0), so  <>[](b = 1)  is VIOLATED; the cycle of the counterexample passes b = 0.  (A rule that asked for ALL states of the component to be ~P would let it pass.) *)
EXTENDS Naturals

(* --algorithm stable
variables b = 0;

fair process Flip = 0
begin
  F: while TRUE do
       b := 1 - b;
     end while;
end process

end algorithm *)

Settles == <>[](b = 1)
=============================================================================
